// Minimizer seeding (ba_seeding_*, ba_host.cpp): from the bytes of a problem -- one read against one reference stretch on one strand -- to its
// raw hits, sorted by (reference position, query position): what ba_chaining_create takes. The rule is stated in INTEGRATION.md, "Seeding";
// everything is integer arithmetic, so the kernels equal the model of tests/seeding_ref.py bit for bit.
//
// k_seeding_sketch<EMIT>: the (w, k)-minimizer sketch of every sequence, as a count pass and an emit pass with a scan of the counts between
// them. One wave per sequence at a time, persistent, the sequences longest first through a work counter. The kernel says how a byte is read
// (4: not ACGT; a minus-strand query is read from its end and complemented) and where an entry goes; the loop over the sequence's windows,
// 64 at a time, is sketch_windows of ba_seed_device.hpp, which the index's sketches run as well. A query's entries are also written as sort
// keys, code << 32 | pos.
// k_seeding_sort: one workgroup per problem sorts the query's keys with a normalized bitonic network: every compare-exchange is ascending,
// so an entry past the end would never move, and a pair whose partner lies past the end is skipped: no padding. Up to 8192 entries in LDS,
// more than that in the problem's own slice of global memory, the same network between workgroup barriers.
// k_seeding_match<EMIT>: one wave per problem, 64 reference entries per step, again a count pass, a scan and an emit pass. Every lane
// searches the lower and the upper bound of its code among the query's sorted keys; a count above max_occ becomes 0; a prefix sum over the
// wave and a running base give the place of the entry's hits.
#include <hip/hip_runtime.h>

#include "ba_launch.h"
#include "ba_seed_device.hpp"

using namespace ba::seed;   // the helpers shared with ba_index.hip and ba_index_both.hip

namespace {

constexpr uint32_t SKETCH_WAVES = 4, MATCH_WAVES = 4, SORT_THREADS = 1024;

}  // namespace

template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_seeding_sketch(const ba::SeedingParams sp) {
    __shared__ SketchLds lds[SKETCH_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    SketchLds& L = lds[threadIdx.x >> 6];
    const uint32_t k = sp.k, w = sp.w, n_seq = 2u * sp.n;
    for (;;) {
        const uint32_t t = next_work(sp.counter, lane);
        if (t >= n_seq) break;
        const uint32_t s = sp.seq_order[t], len = sp.seq_len[s];
        const uint8_t* seq = sp.pool + sp.seq_off[s];
        const bool rc = sp.seq_rc[s] != 0;
        const uint32_t nk = len >= k ? len - k + 1u : 0u;                  // k-mers
        const uint32_t nw = nk == 0u ? 0u : nk > w ? nk - w + 1u : 1u;     // windows
        const uint64_t out0 = EMIT ? sp.seed_first[s] : 0ull;
        const auto two = [&](uint32_t i) { return i < len ? two_bits(seq[rc ? len - 1u - i : i], rc) : 4u; };
        const uint32_t count = sketch_windows<false, EMIT>(L, two, 0u, nw, k, w, nk, NO_KEY, lane, [&](uint32_t i, uint32_t code, uint32_t pos) {
            const uint64_t at = out0 + i;
            sp.seed_pos[at] = pos; sp.seed_code[at] = code;
            if (s < sp.n) sp.q_key[at] = (uint64_t)code << 32 | pos;   // (the queries' entries come first: the same index)
        });
        if (!EMIT && lane == 0) sp.seed_cnt[s] = count;
    }
}

__global__ void __launch_bounds__(SORT_THREADS) k_seeding_sort(const ba::SeedingParams sp) {
    __shared__ uint64_t keys[ba::SEEDING_SORT_LDS];
    for (uint32_t t = blockIdx.x; t < sp.n; t += gridDim.x) {
        const uint32_t p = sp.sort_order[t];
        const uint64_t a0 = sp.seed_first[p];
        const uint32_t cnt = (uint32_t)(sp.seed_first[p + 1] - a0);
        uint64_t* g = sp.q_key + a0;
        if (cnt < 2u) continue;
        if (cnt <= ba::SEEDING_SORT_LDS) {
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) keys[i] = g[i];
            __syncthreads();
            sort_network<SORT_THREADS>(keys, cnt);
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) g[i] = keys[i];
            __syncthreads();   // the next problem overwrites the keys
        } else {
            sort_network<SORT_THREADS>(g, cnt);   // (__syncthreads orders the workgroup's global accesses as well)
        }
    }
}

template <bool EMIT> __global__ void __launch_bounds__(64 * MATCH_WAVES) k_seeding_match(const ba::SeedingParams sp) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x * MATCH_WAVES + wv; t < sp.n; t += gridDim.x * MATCH_WAVES) {
        const uint32_t p = sp.match_order[t];
        const uint64_t q0 = sp.seed_first[p], r0 = sp.seed_first[sp.n + p];
        const uint32_t qc = (uint32_t)(sp.seed_first[p + 1] - q0), rcnt = (uint32_t)(sp.seed_first[sp.n + p + 1] - r0);
        const uint64_t* qk = sp.q_key + q0;
        const uint64_t h0 = EMIT ? sp.hit_first[p] : 0ull;
        uint64_t total = 0;   // the lane's own hits (the count pass)
        uint32_t run = 0;     // the hits of the steps before (the emit pass: at most 2^28 in all)
        for (uint32_t base = 0; base < rcnt; base += 64u) {
            const uint32_t e = base + lane;
            uint32_t m = 0, lo = 0;
            if (e < rcnt && qc) {
                const uint64_t code = sp.seed_code[r0 + e];
                lo = lower_bound(qk, qc, code << 32);
                if (lo < qc && qk[lo] >> 32 == code) {   // (most codes of a reference are not in the query: no second search for them)
                    // (the end of the code's run: no position is 0xffffffff; code + 1 would leave 64 bits for the all-T 16-mer)
                    m = 1u + lower_bound(qk + lo + 1u, qc - lo - 1u, code << 32 | 0xffffffffull);
                    if (m > sp.max_occ) m = 0;
                }
            }
            if (EMIT) {
                const uint32_t incl = wave_incl_sum(m, lane);
                if (m) {
                    const uint64_t at = h0 + run + (incl - m);
                    const uint32_t rpos = sp.seed_pos[r0 + e];
                    for (uint32_t i = 0; i < m; i++) { sp.q_hit[at + i] = (uint32_t)qk[lo + i]; sp.r_hit[at + i] = rpos; sp.hit_len[at + i] = sp.k; }
                }
                run += bcast(incl, 63);
            } else {
                total += m;
            }
        }
        if (!EMIT) {
            total = wave_sum64(total);
            if (lane == 0) sp.hit_cnt[p] = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
        }
    }
}

// The sketch's count pass (emit 0: seed_cnt) or emit pass (seed_pos, seed_code, q_key at seed_first); the work counter is zeroed by the host.
extern "C" hipError_t ba_launch_seeding_sketch(hipStream_t s, const ba::SeedingParams* sp, int emit) {
    const uint32_t wgs = (2u * sp->n + SKETCH_WAVES - 1u) / SKETCH_WAVES;
    const dim3 grid(wgs < 2048u ? wgs : 2048u), block(64 * SKETCH_WAVES);
    if (emit) k_seeding_sketch<true><<<grid, block, 0, s>>>(*sp);
    else k_seeding_sketch<false><<<grid, block, 0, s>>>(*sp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_seeding_sort(hipStream_t s, const ba::SeedingParams* sp) {
    k_seeding_sort<<<dim3(sp->n < 2048u ? sp->n : 2048u), dim3(SORT_THREADS), 0, s>>>(*sp);
    return hipGetLastError();
}
// The match's count pass (emit 0: hit_cnt) or emit pass (q_hit, r_hit, hit_len at hit_first).
extern "C" hipError_t ba_launch_seeding_match(hipStream_t s, const ba::SeedingParams* sp, int emit) {
    const uint32_t wgs = (sp->n + MATCH_WAVES - 1u) / MATCH_WAVES;
    const dim3 grid(wgs < 4096u ? wgs : 4096u), block(64 * MATCH_WAVES);
    if (emit) k_seeding_match<true><<<grid, block, 0, s>>>(*sp);
    else k_seeding_match<false><<<grid, block, 0, s>>>(*sp);
    return hipGetLastError();
}
