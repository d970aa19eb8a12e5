// The reference index (ba_ref_index_*, ba_seeding_create_indexed; ba_host.cpp): the sketch of one long reference, built once, and the
// lookup of many reads in it. The rule is stated in INTEGRATION.md, "Reference index": "Seeding"'s rule with r the whole reference, plus a
// cap on the occurrences of a code in the reference's sketch. Everything is integer arithmetic, so the kernels equal the model of
// tests/index_ref.py bit for bit. The sort of the index's keys is a library call in a unit of its own (ba_index_sort.hip).
//
// k_index_sketch<EMIT>: k_seeding_sketch's count and emit passes for sequences that many waves share. A work item is a span of
// INDEX_SPAN windows of one sequence, taken from a work counter; within it the wave goes chunk by chunk as k_seeding_sketch does. The one
// new thing is the seam: a window's minimizer is selected when it differs from the window's before it, so a span that does not start its
// sequence first computes the minimizer of the window before its first one from the w k-mers under that window -- all ones when none of
// them is valid, which is also what a sequence's first window compares with. The entries are written as keys code << 32 | pos, in position
// order. Several sequences ("Several sequences" in INTEGRATION.md) lie end to end in one frame; the host numbers every sequence's spans
// from seq_span[s], the wave finds its span's sequence by a lower bound over those, and every byte outside that sequence reads as invalid:
// one reference is the case n_seqs = 1, with the same arithmetic.
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
static_assert(ba::INDEX_SPAN % 64u == 0u, "a span is whole chunks");

}  // namespace

template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_index_sketch(const ba::IndexParams ip) {
    __shared__ SketchLds lds[SKETCH_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    SketchLds& L = lds[threadIdx.x >> 6];
    const uint32_t k = ip.k, w = ip.w;
    for (;;) {
        __builtin_amdgcn_wave_barrier();   // (a convergence point, as in k_seeding_sketch)
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ip.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= ip.n_spans) break;
        // the span's sequence: the last one whose first span is t or before it (a sequence without a k-mer has no span, so it is never that)
        const uint32_t sq = lower_bound(ip.seq_span, ip.n_seqs + 1u, (uint64_t)t + 1u) - 1u;
        const uint32_t S = (uint32_t)ip.seq_start[sq], E = (uint32_t)ip.seq_start[sq + 1u];   // its bytes, in the index's frame (E - S >= k)
        const uint32_t nk = E - k + 1u;   // one past its last k-mer; positions, k-mers and windows are numbered in the index's frame from here on
        const uint32_t nw = nk - S > w ? nk - w + 1u : S + 1u;   // one past its last window
        const auto two = [&](uint32_t i) { return i >= S && i < E ? two_bits(ip.ref[i], false) : 4u; };   // (no byte of a neighbour)
        const uint32_t first = S + (t - (uint32_t)ip.seq_span[sq]) * ba::INDEX_SPAN, last = first + ba::INDEX_SPAN < nw ? first + ba::INDEX_SPAN : nw;
        uint64_t prev = NO_KEY;   // the minimizer of the window before the chunk
        if (first != S) {         // the seam: window first - 1 lies over the k-mers first - 1 .. first + w - 2 (the sequence has more than w here)
            for (uint32_t b = lane; b < w + k - 1u; b += 64u) L.two[b] = (uint8_t)two(first - 1u + b);
            wave_sync();
            uint32_t code;
            prev = wave_min64(lane < w ? kmer_key(L, lane, first - 1u + lane, k, nk, code) : NO_KEY);
            wave_sync();   // the first chunk overwrites what this read
        }
        const uint64_t out0 = EMIT ? ip.span_first[t] : 0ull;
        uint32_t count = 0;
        for (uint32_t s0 = first; s0 < last; s0 += 64u) {
            const uint64_t m = chunk_minimizer(L, two, s0, last, k, w, nk, lane);   // (a window past the span's last one is the next span's)
            const bool take = chunk_select(m, prev, lane);
            const uint64_t ballot = __ballot(take);
            if (EMIT && take) {
                const uint32_t pos = (uint32_t)m;
                ip.unsorted[out0 + count + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint64_t)L.code[pos - s0] << 32 | pos;
            }
            count += (uint32_t)__popcll(ballot);
            wave_sync();   // the next chunk overwrites what this one read
        }
        if (!EMIT && lane == 0) ip.span_cnt[t] = count;
    }
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
