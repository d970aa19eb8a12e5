// The reference index (ba_ref_index_*, ba_seeding_create_indexed; ba_host.cpp): the sketch of one long reference, built once, and the
// lookup of many reads in it. The rule is stated in INTEGRATION.md, "Reference index": "Seeding"'s rule with r the whole reference, plus a
// cap on the occurrences of a code in the reference's sketch. Everything is integer arithmetic, so the kernels equal the model of
// tests/index_ref.py bit for bit. The sort of the index's keys is a library call in a unit of its own (ba_index_sort.hip).
//
// k_index_sketch<EMIT>: k_seeding_sketch's count and emit passes for sequences that many waves share. A work item is a span of
// INDEX_SPAN windows of one sequence, taken from a work counter; within it the wave goes chunk by chunk as k_seeding_sketch does, after
// the seam: the minimizer of the window before the span. The entries are written as keys code << 32 | pos, in position order. Several
// sequences ("Several sequences" in INTEGRATION.md) lie end to end in one frame, and every byte outside a span's sequence reads as
// invalid. The body is index_sketch<false, EMIT> of ba_seed_device.hpp, which says all this in full; the canonical index
// (ba_index_both.hip) runs the same body over canonical k-mers.
// k_index_table: one lower bound per prefix over the sorted keys, and the longest run of one code, by a search from every run's start.
// k_index_lookup<EMIT>: one wave per problem, longest query first, 64 of the query's sorted keys per step, a count pass, a scan and an emit
// pass. Every lane finds how often its code occurs in the query (k_seeding_match's two searches) and, through the prefix table, in the
// index; over either cap the count becomes 0; the emit pass writes keys r_pos << 32 | q_pos at the problem's place.
// k_index_hit_sort: one workgroup per problem sorts those keys -- the order of the rule, (r_hit, q_hit) -- with the normalized bitonic
// network, in LDS or in the problem's slice of global memory as k_seeding_sort, and unpacks them into q_hit, r_hit and hit_len.
#include <hip/hip_runtime.h>

#include "ba_launch.h"
#include "ba_seed_device.hpp"

using namespace ba::seed;

namespace {

constexpr uint32_t SKETCH_WAVES = 4, LOOKUP_WAVES = 4, SORT_THREADS = 1024, TABLE_THREADS = 256;

}  // namespace

template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_index_sketch(const ba::IndexParams ip) {
    __shared__ SketchLds lds[SKETCH_WAVES];
    index_sketch<false, EMIT>(ip, lds[threadIdx.x >> 6]);
}

__global__ void __launch_bounds__(TABLE_THREADS) k_index_table(const ba::IndexParams ip) {
    const uint32_t n = ip.n_entries, slots = (1u << ip.prefix_bits) + 1u;
    const uint32_t shift = 32u + 2u * ip.k - ip.prefix_bits;   // (at most 44: a prefix below 1 << prefix_bits stays inside 64 bits)
    const uint32_t work = n > slots ? n : slots;
    uint32_t longest = 0;
    for (uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x; i < work; i += gridDim.x * TABLE_THREADS) {
        // (one past the last prefix is the end; shifted, it would leave 64 bits for k = 16)
        if (i < slots) ip.table[i] = i == slots - 1u ? n : lower_bound(ip.key, n, (uint64_t)i << shift);
        if (i < n) {
            const uint64_t code = ip.key[i] >> 32;
            if (i == 0u || ip.key[i - 1u] >> 32 != code) {   // a run's start. (No position is 0xffffffff; code + 1 would leave 64 bits.)
                const uint32_t run = 1u + lower_bound(ip.key + i + 1u, n - i - 1u, code << 32 | 0xffffffffull);
                longest = run > longest ? run : longest;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0u && longest) atomicMax(ip.longest_run, longest);
}

template <bool EMIT> __global__ void __launch_bounds__(64 * LOOKUP_WAVES) k_index_lookup(const ba::IndexLookupParams lp) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t shift = 2u * lp.k - lp.prefix_bits;
    const bool q_cap = lp.max_occ != 0xffffffffu;   // (without a cap nobody asks how often the query holds a code)
    for (uint32_t t = blockIdx.x * LOOKUP_WAVES + wv; t < lp.n; t += gridDim.x * LOOKUP_WAVES) {
        const uint32_t p = lp.order[t];
        const uint64_t q0 = lp.seed_first[p];
        const uint32_t qc = (uint32_t)(lp.seed_first[p + 1] - q0);
        const uint64_t* qk = lp.q_key + q0;
        const uint64_t h0 = EMIT ? lp.hit_first[p] : 0ull;
        uint64_t total = 0;   // the lane's own hits (the count pass)
        uint32_t run = 0;     // the hits of the steps before (the emit pass: at most 2^28 in all)
        for (uint32_t base = 0; base < qc; base += 64u) {
            const uint32_t e = base + lane;
            uint32_t m = 0, at_r = 0, qpos = 0;
            if (e < qc) {
                const uint64_t mine = qk[e], code = mine >> 32;
                qpos = (uint32_t)mine;
                uint32_t mq = 1;
                if (q_cap) {   // the code's run among the query's keys: it starts at or before e and ends after it
                    const uint32_t lo = lower_bound(qk, e, code << 32);
                    mq = e + 1u + lower_bound(qk + e + 1u, qc - e - 1u, code << 32 | 0xffffffffull) - lo;
                }
                const uint32_t x = (uint32_t)code >> shift, a = lp.table[x], b = lp.table[x + 1u];
                at_r = a + lower_bound(lp.key + a, b - a, code << 32);
                if (at_r < b && lp.key[at_r] >> 32 == code)
                    m = 1u + lower_bound(lp.key + at_r + 1u, b - at_r - 1u, code << 32 | 0xffffffffull);
                if (mq > lp.max_occ || m > lp.max_ref_occ) m = 0;
            }
            if (EMIT) {
                const uint32_t incl = wave_incl_sum(m, lane);
                const uint64_t at = h0 + run + (incl - m);
                for (uint32_t i = 0; i < m; i++) lp.hit_key[at + i] = lp.key[at_r + i] << 32 | qpos;
                run += bcast(incl, 63);
            } else {
                total += m;
            }
        }
        if (!EMIT) {
            total = wave_sum64(total);
            if (lane == 0) lp.hit_cnt[p] = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
        }
    }
}

__global__ void __launch_bounds__(SORT_THREADS) k_index_hit_sort(const ba::IndexLookupParams lp) {
    __shared__ uint64_t keys[ba::SEEDING_SORT_LDS];
    for (uint32_t t = blockIdx.x; t < lp.n; t += gridDim.x) {
        const uint32_t p = lp.order[t];
        const uint64_t a0 = lp.hit_first[p];
        const uint32_t cnt = (uint32_t)(lp.hit_first[p + 1] - a0);
        uint64_t* g = lp.hit_key + a0;
        if (cnt <= ba::SEEDING_SORT_LDS) {
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) keys[i] = g[i];
            __syncthreads();
            if (cnt >= 2u) sort_network<SORT_THREADS>(keys, cnt);
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) {
                const uint64_t x = keys[i];
                lp.q_hit[a0 + i] = (uint32_t)x; lp.r_hit[a0 + i] = (uint32_t)(x >> 32); lp.hit_len[a0 + i] = lp.k;
            }
            __syncthreads();   // the next problem overwrites the keys
        } else {
            sort_network<SORT_THREADS>(g, cnt);   // (__syncthreads orders the workgroup's global accesses as well)
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) {
                const uint64_t x = g[i];
                lp.q_hit[a0 + i] = (uint32_t)x; lp.r_hit[a0 + i] = (uint32_t)(x >> 32); lp.hit_len[a0 + i] = lp.k;
            }
        }
    }
}

// The sketch's count pass (emit 0: span_cnt) or emit pass (unsorted at span_first); the work counter is zeroed by the host.
extern "C" hipError_t ba_launch_index_sketch(hipStream_t s, const ba::IndexParams* ip, int emit) {
    if (!ip->n_spans) return hipSuccess;
    const uint32_t wgs = (ip->n_spans + SKETCH_WAVES - 1u) / SKETCH_WAVES;
    const dim3 grid(wgs < 2048u ? wgs : 2048u), block(64 * SKETCH_WAVES);
    if (emit) k_index_sketch<true><<<grid, block, 0, s>>>(*ip);
    else k_index_sketch<false><<<grid, block, 0, s>>>(*ip);
    return hipGetLastError();
}
// The prefix table (1 << prefix_bits entries and one more) and longest_run, zeroed by the host, from the sorted keys.
extern "C" hipError_t ba_launch_index_table(hipStream_t s, const ba::IndexParams* ip) {
    const uint32_t slots = (1u << ip->prefix_bits) + 1u, work = ip->n_entries > slots ? ip->n_entries : slots;
    const uint32_t wgs = (work + TABLE_THREADS - 1u) / TABLE_THREADS;
    k_index_table<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(TABLE_THREADS), 0, s>>>(*ip);
    return hipGetLastError();
}
// The lookup's count pass (emit 0: hit_cnt) or emit pass (hit_key at hit_first).
extern "C" hipError_t ba_launch_index_lookup(hipStream_t s, const ba::IndexLookupParams* lp, int emit) {
    const uint32_t wgs = (lp->n + LOOKUP_WAVES - 1u) / LOOKUP_WAVES;
    const dim3 grid(wgs < 4096u ? wgs : 4096u), block(64 * LOOKUP_WAVES);
    if (emit) k_index_lookup<true><<<grid, block, 0, s>>>(*lp);
    else k_index_lookup<false><<<grid, block, 0, s>>>(*lp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_index_hit_sort(hipStream_t s, const ba::IndexLookupParams* lp) {
    k_index_hit_sort<<<dim3(lp->n < 2048u ? lp->n : 2048u), dim3(SORT_THREADS), 0, s>>>(*lp);
    return hipGetLastError();
}
