// Both strands at once (ba_ref_index_create_canonical, ba_seeding_create_indexed_both; ba_host.cpp): a canonical reference index and the
// lookup of reads in it, each read sketched once and seeded on both strands. The rule is stated in INTEGRATION.md, "Both strands at once":
// "Reference index"'s rule on canonical codes -- the smaller of a k-mer's code and its reverse complement's, with one bit for which one it
// was in bit 31 of a key's low word, which every position leaves free. Everything is integer arithmetic, so the kernels equal the model of
// tests/index_both_ref.py bit for bit. The kernels of ba_index.hip and ba_seeding.hip that do not look at a key's low word -- the sort of a
// read's keys, the library sort of the index, the prefix table and the sort of the hits -- are launched as they are.
//
// The two sketches are the plain ones' code (ba_seed_device.hpp) with CANON set: the same work counter, chunk loop and selection.
// k_both_index_sketch<EMIT>: k_index_sketch's body, index_sketch, over canonical k-mers; an entry is written as
// code << 32 | strand << 31 | pos.
// k_both_read_sketch<EMIT>: k_seeding_sketch's persistent wave per read and its loop, sketch_windows, over the n reads only and always
// forward: seed_pos holds the strand in bit 31, and q_key is an index key in the read's own frame.
// k_both_lookup<EMIT>: k_index_lookup's wave per read and 64 sorted read entries per step. A lane finds its code's run among the read's keys
// and, through the prefix table, in the index, both strands together for the caps; one more search splits the index's run into its strand-0
// and strand-1 entries. An index entry on the lane's own strand is a hit of problem 2 r, one on the other strand a hit of problem 2 r + 1
// whose query position is the k-mer's start in the read's reverse complement. Two counts, two prefix sums and two running bases.
#include <hip/hip_runtime.h>

#include "ba_launch.h"
#include "ba_seed_device.hpp"

using namespace ba::seed;

namespace {

constexpr uint32_t SKETCH_WAVES = 4, LOOKUP_WAVES = 4;

}  // namespace

template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_both_index_sketch(const ba::IndexParams ip) {
    __shared__ CanonLds lds[SKETCH_WAVES];
    index_sketch<true, EMIT>(ip, lds[threadIdx.x >> 6]);
}

// sp.n: the reads; sp.seq_off, sp.seq_len and sp.seq_order are theirs (n each), and no sequence is a reference's.
template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_both_read_sketch(const ba::SeedingParams sp) {
    __shared__ CanonLds lds[SKETCH_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    CanonLds& L = lds[threadIdx.x >> 6];
    const uint32_t k = sp.k, w = sp.w;
    for (;;) {
        const uint32_t t = next_work(sp.counter, lane);
        if (t >= sp.n) break;
        const uint32_t s = sp.seq_order[t], len = sp.seq_len[s];
        const uint8_t* seq = sp.pool + sp.seq_off[s];
        const uint32_t nk = len >= k ? len - k + 1u : 0u;                  // k-mers
        const uint32_t nw = nk == 0u ? 0u : nk > w ? nk - w + 1u : 1u;     // windows
        const uint64_t out0 = EMIT ? sp.seed_first[s] : 0ull;
        const auto two = [&](uint32_t i) { return i < len ? two_bits(seq[i], false) : 4u; };   // (a read is never reversed for its sketch)
        const uint32_t count = sketch_windows<true, EMIT>(L, two, 0u, nw, k, w, nk, NO_KEY, lane, [&](uint32_t i, uint32_t code, uint32_t low) {
            const uint64_t at = out0 + i;
            sp.seed_pos[at] = low; sp.seed_code[at] = code;
            sp.q_key[at] = (uint64_t)code << 32 | low;
        });
        if (!EMIT && lane == 0) sp.seed_cnt[s] = count;
    }
}

template <bool EMIT> __global__ void __launch_bounds__(64 * LOOKUP_WAVES) k_both_lookup(const ba::IndexBothParams bp) {
    const ba::IndexLookupParams& lp = bp.lp;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t shift = 2u * lp.k - lp.prefix_bits;
    const bool q_cap = lp.max_occ != 0xffffffffu;   // (without a cap nobody asks how often the read holds a code)
    for (uint32_t t = blockIdx.x * LOOKUP_WAVES + wv; t < lp.n; t += gridDim.x * LOOKUP_WAVES) {
        const uint32_t r = lp.order[t];
        const uint64_t q0 = lp.seed_first[r];
        const uint32_t qc = (uint32_t)(lp.seed_first[r + 1] - q0);
        const uint32_t flip = bp.q_len[r] - lp.k;   // (a read with an entry has at least k bytes)
        const uint64_t* qk = lp.q_key + q0;
        const uint64_t h0 = EMIT ? lp.hit_first[2u * r] : 0ull, h1 = EMIT ? lp.hit_first[2u * r + 1u] : 0ull;
        uint64_t total0 = 0, total1 = 0;   // the lane's own hits per problem (the count pass)
        uint32_t run0 = 0, run1 = 0;       // the hits of the steps before (the emit pass: at most 2^28 in all)
        for (uint32_t base = 0; base < qc; base += 64u) {
            const uint32_t e = base + lane;
            uint32_t m0 = 0, m1 = 0, at_r = 0, n0 = 0, m = 0, qpos = 0, sq = 0;   // m0, m1: the lane's hits on its own and on the other strand
            if (e < qc) {
                const uint64_t mine = qk[e], code = mine >> 32;
                qpos = (uint32_t)mine & ba::INDEX_POS_MASK;
                sq = (uint32_t)mine >> 31;
                uint32_t mq = 1;
                if (q_cap) {   // the code's run among the read's keys, both strands together: it starts at or before e and ends after it
                    const uint32_t lo = lower_bound(qk, e, code << 32);
                    mq = e + 1u + lower_bound(qk + e + 1u, qc - e - 1u, code << 32 | 0xffffffffull) - lo;
                }
                const uint32_t x = (uint32_t)code >> shift, a = lp.table[x], b = lp.table[x + 1u];
                at_r = a + lower_bound(lp.key + a, b - a, code << 32);
                if (at_r < b && lp.key[at_r] >> 32 == code) {   // (no low word is 0xffffffff: a position stays below 2^31 - 16)
                    m = 1u + lower_bound(lp.key + at_r + 1u, b - at_r - 1u, code << 32 | 0xffffffffull);
                    n0 = lower_bound(lp.key + at_r, m, code << 32 | ba::INDEX_STRAND_BIT);   // the run's strand-0 entries come first
                }
                if (mq > lp.max_occ || m > lp.max_ref_occ) m = 0, n0 = 0;
                m0 = sq ? m - n0 : n0;
                m1 = m - m0;
            }
            if (EMIT) {
                const uint32_t incl0 = wave_incl_sum(m0, lane), incl1 = wave_incl_sum(m1, lane);
                // the index's strand-0 entries, then its strand-1 entries: each group is on the lane's own strand or on the other one
                const uint64_t at0 = h0 + run0 + (incl0 - m0), at1 = h1 + run1 + (incl1 - m1);
                const uint64_t same = sq ? at1 : at0, other = sq ? at0 : at1;   // where the hits against strand-0 entries go, and the rest
                const uint32_t q_same = sq ? flip - qpos : qpos, q_other = sq ? qpos : flip - qpos;
                for (uint32_t i = 0; i < n0; i++) lp.hit_key[same + i] = (lp.key[at_r + i] & ba::INDEX_POS_MASK) << 32 | q_same;
                for (uint32_t i = n0; i < m; i++) lp.hit_key[other + (i - n0)] = (lp.key[at_r + i] & ba::INDEX_POS_MASK) << 32 | q_other;
                run0 += bcast(incl0, 63);
                run1 += bcast(incl1, 63);
            } else {
                total0 += m0;
                total1 += m1;
            }
        }
        if (!EMIT) {
            total0 = wave_sum64(total0);
            total1 = wave_sum64(total1);
            if (lane == 0) {
                lp.hit_cnt[2u * r] = total0 > 0xffffffffull ? 0xffffffffu : (uint32_t)total0;
                lp.hit_cnt[2u * r + 1u] = total1 > 0xffffffffull ? 0xffffffffu : (uint32_t)total1;
            }
        }
    }
}

// The canonical index sketch's count pass (emit 0: span_cnt) or emit pass (unsorted at span_first); the work counter is zeroed by the host.
extern "C" hipError_t ba_launch_both_index_sketch(hipStream_t s, const ba::IndexParams* ip, int emit) {
    if (!ip->n_spans) return hipSuccess;
    const uint32_t wgs = (ip->n_spans + SKETCH_WAVES - 1u) / SKETCH_WAVES;
    const dim3 grid(wgs < 2048u ? wgs : 2048u), block(64 * SKETCH_WAVES);
    if (emit) k_both_index_sketch<true><<<grid, block, 0, s>>>(*ip);
    else k_both_index_sketch<false><<<grid, block, 0, s>>>(*ip);
    return hipGetLastError();
}
// The reads' sketch: the count pass (emit 0: seed_cnt) or the emit pass (seed_pos, seed_code, q_key at seed_first), over sp->n reads.
extern "C" hipError_t ba_launch_both_read_sketch(hipStream_t s, const ba::SeedingParams* sp, int emit) {
    const uint32_t wgs = (sp->n + SKETCH_WAVES - 1u) / SKETCH_WAVES;
    const dim3 grid(wgs < 2048u ? wgs : 2048u), block(64 * SKETCH_WAVES);
    if (emit) k_both_read_sketch<true><<<grid, block, 0, s>>>(*sp);
    else k_both_read_sketch<false><<<grid, block, 0, s>>>(*sp);
    return hipGetLastError();
}
// The lookup's count pass (emit 0: hit_cnt of both problems of a read) or emit pass (hit_key at their hit_first).
extern "C" hipError_t ba_launch_both_lookup(hipStream_t s, const ba::IndexBothParams* bp, int emit) {
    const uint32_t wgs = (bp->lp.n + LOOKUP_WAVES - 1u) / LOOKUP_WAVES;
    const dim3 grid(wgs < 4096u ? wgs : 4096u), block(64 * LOOKUP_WAVES);
    if (emit) k_both_lookup<true><<<grid, block, 0, s>>>(*bp);
    else k_both_lookup<false><<<grid, block, 0, s>>>(*bp);
    return hipGetLastError();
}
