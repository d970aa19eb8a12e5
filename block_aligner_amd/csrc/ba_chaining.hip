// Colinear anchor chaining (ba_chaining_*, ba_host.cpp): from the raw hits of a problem -- one read against one reference on one strand,
// sorted by (reference end, query end) -- to the best colinear chains, in the layout ba_chain_batch_create takes. The rule is stated in
// INTEGRATION.md, "Chaining anchors"; everything is integer arithmetic, so the kernels equal the model of tests/chaining_ref.py bit for bit.
//
// k_chaining_fill: the recurrence. One wave per problem at a time, persistent, the problems longest first through a work counter. The wave
// loads 64 anchors at once, one per lane, and takes them one after the other (v_readlane broadcasts the anchor). The (qe, re, f) of the
// anchors behind sit in an LDS ring of a power of two >= H + 64 slots: qe and re of a whole chunk are written when it is loaded -- the slots
// they take are more than H behind every anchor of the chunk --, f when its anchor is done. The look-back of an anchor runs across the
// lanes, lane l looking at j = i - 1 - l, - 65 - l, ..., and every lane keeps the maximum of a packed key (v biased to unsigned, j); "no
// predecessor" is the key (match_w L, 0xffffffff), so that on equal v "none" beats every j and a nearer j a farther one: one DPP max
// reduction over the 64 keys per anchor gives f and pred at once, and the lane that holds the winning key the gain.
// k_chaining_pick: one wave per problem. Per candidate a wave-wide arg-max of f over the anchors no walk has taken, then the walk along pred,
// 64 anchors per load, which marks every anchor with the candidate and its place counted from the end.
// k_chaining_gather: one wave per problem. A candidate per lane: ranks and offsets of the kept ones by a ballot and a prefix sum; then every
// marked anchor of a kept chain goes to its final place, trimmed to its gain.
#include <hip/hip_runtime.h>

#include "ba_launch.h"
#include "ba_seed_device.hpp"   // (lower_bound)

// One source, two units: BA_CHAINING_UNIT 0 (the default) holds the three kernels of a chainer, 1 the fill of a chainer bounded by a
// sequence table (k_chaining_fill<true>, ba_launch_chaining_fill_bounded) and nothing else -- so the unit that every chainer without a
// table runs is built from what it was built from before there were tables.
#ifndef BA_CHAINING_UNIT
#define BA_CHAINING_UNIT 0
#endif

namespace {

constexpr uint32_t NONE = ba::CHAINING_NONE;
constexpr uint32_t BIAS = 0x80000000u;   // int32 -> uint32, order kept

// lanes of one wave hand data to one another through memory: program order is enough for the hardware (a wave's LDS operations run in
// order), the compiler must keep it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// x = max(x, x of the lane the DPP control names); lanes without a source, and rows outside ROWS, keep x
template <int CTRL, int ROWS> __device__ __forceinline__ uint64_t dpp_max(uint64_t x) {
    const int lo = (int)(uint32_t)x, hi = (int)(uint32_t)(x >> 32);
    const uint32_t ol = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xf, false);
    const uint32_t oh = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xf, false);
    const uint64_t y = (uint64_t)oh << 32 | ol;
    return y > x ? y : x;
}
// the maximum over the wave, in every lane (a scalar): row_shr 1, 2, 4, 8 leave a row's maximum in its lane 15, row_bcast:15 / :31 carry it
// on to lane 63
__device__ __forceinline__ uint64_t wave_max(uint64_t x) {
    x = dpp_max<0x111, 0xf>(x);
    x = dpp_max<0x112, 0xf>(x);
    x = dpp_max<0x114, 0xf>(x);
    x = dpp_max<0x118, 0xf>(x);
    x = dpp_max<0x142, 0xa>(x);
    x = dpp_max<0x143, 0xc>(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint32_t bcast(uint32_t x, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)lane); }
__device__ __forceinline__ uint32_t shfl(uint32_t x, uint32_t src) { return (uint32_t)__shfl((int)x, (int)src, 64); }
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= (uint32_t)d ? o : 0u;
    }
    return x;
}

}  // namespace

// BOUNDED: the anchors lie in the frame of several sequences laid end to end ("Several sequences" in INTEGRATION.md), and a chain stays
// inside one: the lane that loads an anchor finds S, the start of the sequence that holds it, by a lower bound over seq_start, and a
// predecessor must end behind S -- the anchors are sorted by their ends and none straddles a junction, so that is exactly a predecessor in
// the anchor's own sequence. re_j > S is dr = re_i - re_j < re_i - S, a bound on dr beside max_dist: the lane turns S into the anchor's own
// limit min(max_dist, re_i - S - 1), which goes round with the anchor, and the look-back compares dr with it where it compared with
// max_dist -- no instruction more per predecessor. Without BOUNDED none of this is compiled.
template <bool BOUNDED> __global__ void __launch_bounds__(256) k_chaining_fill(const ba::ChainingParams cp) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, mask = cp.ring - 1u;
    uint32_t* rq = lds + w * 3u * cp.ring;
    uint32_t* rr = rq + cp.ring;
    int32_t* rf = (int32_t*)(rr + cp.ring);
    const uint32_t mw = (uint32_t)cp.match_w, dc = (uint32_t)cp.drift_cost, sc = (uint32_t)cp.skip_cost;
    for (;;) {
        const uint32_t k = ba::seed::next_work(cp.counter, lane);
        if (k >= cp.n) break;
        const uint32_t p = cp.order[k];
        const uint64_t a0 = cp.anchor_first[p];
        const uint32_t cnt = (uint32_t)(cp.anchor_first[p + 1] - a0);
        for (uint32_t base = 0; base < cnt; base += 64u) {
            const uint32_t il = base + lane;
            const bool in = il < cnt;
            uint32_t L = 1, qe = 0, re = 0, lim = 0;   // lim (BOUNDED): the largest dr a predecessor of the anchor may have
            if (in) { L = cp.anchor_len[a0 + il]; qe = cp.q_anchor[a0 + il] + L; re = cp.r_anchor[a0 + il] + L; }
            if (BOUNDED && in) {
                // the last sequence that starts at or before the anchor; an empty one starts where the next does, so it is never the last
                const uint32_t S = (uint32_t)cp.seq_start[ba::seed::lower_bound(cp.seq_start, cp.n_seqs + 1u, (uint64_t)(re - L) + 1u) - 1u];
                const uint32_t room = re - S - 1u;   // (re > S: the anchor starts at or behind S and has a base)
                lim = room < cp.max_dist ? room : cp.max_dist;
            }
            // (the slots written held the anchors il - ring <= base + 63 - (H + 64) < base - H: behind every look-back of this chunk)
            rq[il & mask] = qe; rr[il & mask] = re;
            wave_sync();
            int32_t my_f = 0;
            uint32_t my_pred = NONE, my_gain = 0;
            const uint32_t steps = cnt - base < 64u ? cnt - base : 64u;
            for (uint32_t t = 0; t < steps; t++) {
                const uint32_t i = base + t;
                const uint32_t qi = bcast(qe, t), ri = bcast(re, t), Li = bcast(L, t);
                const uint32_t max_dr = BOUNDED ? bcast(lim, t) : cp.max_dist;
                uint64_t key = (uint64_t)((mw * Li) ^ BIAS) << 32 | NONE;
                uint32_t g_key = Li;   // the gain that goes with the lane's key
                const uint32_t look = i < cp.lookback ? i : cp.lookback;
                for (uint32_t o = lane; o < look; o += 64u) {
                    const uint32_t j = i - 1u - o, s = j & mask;
                    const uint32_t udq = qi - rq[s], udr = ri - rr[s];
                    const int32_t dq = (int32_t)udq, dr = (int32_t)udr;
                    const uint32_t fj = (uint32_t)rf[s];
                    const uint32_t drift = dq > dr ? udq - udr : udr - udq, lo = dq < dr ? udq : udr;
                    const uint32_t g = Li < lo ? Li : lo;
                    const bool ok = dq > 0 && dr > 0 && udq <= cp.max_dist && udr <= max_dr && drift <= cp.bandwidth;
                    const uint32_t v = fj + mw * g - dc * drift - sc * (lo - g);   // (an admissible j: no step leaves int32, by the host's checks)
                    const uint64_t cand = (uint64_t)(v ^ BIAS) << 32 | j;
                    if (ok && cand > key) { key = cand; g_key = g; }
                }
                const uint64_t best = wave_max(key);
                const uint32_t pj = (uint32_t)best;
                const int32_t fi = (int32_t)((uint32_t)(best >> 32) ^ BIAS);
                // what is left of anchor i behind its predecessor: from the lane that found it (one lane per j; "none" is every lane's, with L_i)
                const uint32_t gi = bcast(g_key, (uint32_t)__builtin_ctzll(__ballot(key == best)));
                if (lane == 0) rf[i & mask] = fi;
                if (lane == t) { my_f = fi; my_pred = pj; my_gain = gi; }
                wave_sync();
            }
            if (in) { cp.f[a0 + il] = my_f; cp.pred[a0 + il] = my_pred; cp.gain[a0 + il] = my_gain; }
        }
    }
}

#if BA_CHAINING_UNIT == 0

constexpr uint32_t CHAINING_WAVES = 4;   // waves per workgroup of k_chaining_pick and k_chaining_gather: one problem per wave at a time

__global__ void __launch_bounds__(64 * CHAINING_WAVES) k_chaining_pick(const ba::ChainingParams cp) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t k = blockIdx.x * CHAINING_WAVES + w; k < cp.n; k += gridDim.x * CHAINING_WAVES) {
        const uint32_t p = cp.order[k];
        const uint64_t a0 = cp.anchor_first[p];
        const uint32_t cnt = (uint32_t)(cp.anchor_first[p + 1] - a0);
        const int32_t* f = cp.f + a0;
        const uint32_t* pred = cp.pred + a0;
        uint32_t* mark = cp.mark + a0;
        uint32_t* pos = cp.pos + a0;
        for (uint32_t i = lane; i < cnt; i += 64u) mark[i] = NONE;
        __threadfence();   // the marks go from lane to lane through global memory: here, and after every walk
        uint32_t my_len = 0, chains = 0, kept = 0;
        int32_t my_score = 0;
        for (uint32_t c = 0; c < cp.max_chains; c++) {
            uint64_t key = 0;   // (f >= match_w >= 1: a key of an anchor is never 0)
            for (uint32_t i = lane; i < cnt; i += 64u)
                if (mark[i] == NONE) {
                    const uint64_t cand = (uint64_t)((uint32_t)f[i] ^ BIAS) << 32 | (0xffffffffu - i);   // the largest f, then the smallest index
                    if (cand > key) key = cand;
                }
            key = wave_max(key);
            if (key == 0) break;
            const uint32_t e = 0xffffffffu - (uint32_t)key;
            const int32_t fe = (int32_t)((uint32_t)(key >> 32) ^ BIAS);
            if (fe < cp.min_score) break;
            // The walk. pred[i] lies less than H behind i, mostly a few anchors: the wave loads pred and mark of the 64 anchors up to cur at
            // once, follows pred inside that window by v_readlane, and loads again when the walk leaves it. A walk only goes down, so the
            // marks it reads are earlier walks'; its own go out once per window, from the lanes whose anchors it took.
            uint32_t cur = e, len = 0;
            int32_t score = fe;
            for (bool more = true; more;) {
                const uint32_t base = cur >= 63u ? cur - 63u : 0u, idx = base + lane;
                const bool have = idx <= cur;
                const uint32_t wp = have ? pred[idx] : NONE, wm = have ? mark[idx] : NONE;
                uint32_t my_pos = NONE;
                for (;;) {
                    const uint32_t l = cur - base;
                    if (bcast(wm, l) != NONE) { score = fe - f[cur]; more = false; break; }   // a used anchor: the chain is cut behind it
                    if (lane == l) my_pos = len;
                    len++;
                    const uint32_t pj = bcast(wp, l);
                    if (pj == NONE) { more = false; break; }
                    cur = pj;
                    if (pj < base) break;
                }
                if (my_pos != NONE) { mark[idx] = c; pos[idx] = my_pos; }
            }
            __threadfence();
            const bool keep = score >= cp.min_score && len >= cp.min_anchors;
            if (lane == c) { my_len = keep ? len : 0u; my_score = score; }
            if (keep) { chains++; kept += len; }
        }
        if (lane < cp.max_chains) { cp.cand_len[(uint64_t)p * cp.max_chains + lane] = my_len; cp.cand_score[(uint64_t)p * cp.max_chains + lane] = my_score; }
        if (lane == 0) { cp.n_chains[p] = chains; cp.n_kept[p] = kept; }
    }
}

__global__ void __launch_bounds__(64 * CHAINING_WAVES) k_chaining_gather(const ba::ChainingParams cp) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t p = blockIdx.x * CHAINING_WAVES + w; p < cp.n; p += gridDim.x * CHAINING_WAVES) {
        const uint64_t a0 = cp.anchor_first[p];
        const uint32_t cnt = (uint32_t)(cp.anchor_first[p + 1] - a0);
        const uint64_t c0 = cp.chain_off[p], k0 = cp.kept_off[p];
        const uint32_t len = lane < cp.max_chains ? cp.cand_len[(uint64_t)p * cp.max_chains + lane] : 0u;   // lane = candidate
        const uint32_t aoff = wave_incl_sum(len, lane) - len;
        const uint32_t rank = (uint32_t)__popcll(__ballot(len != 0u) & ((1ull << lane) - 1ull));
        if (len) {
            const uint64_t c = c0 + rank;
            cp.chain_problem[c] = p; cp.chain_rank[c] = rank; cp.chain_score[c] = cp.cand_score[(uint64_t)p * cp.max_chains + lane];
            cp.out_first[c] = k0 + aoff;
        }
        if (p == cp.n - 1u && lane == 0) cp.out_first[cp.chain_off[cp.n]] = cp.kept_off[cp.n];
        for (uint32_t base = 0; base < cnt; base += 64u) {
            const uint32_t i = base + lane;
            const uint32_t m = i < cnt ? cp.mark[a0 + i] : NONE;
            const uint32_t from = m == NONE ? 0u : m;
            const uint32_t clen = shfl(len, from), coff = shfl(aoff, from);
            if (m != NONE && clen) {
                const uint64_t at = k0 + coff + (clen - 1u - cp.pos[a0 + i]);
                const uint32_t L = cp.anchor_len[a0 + i], g = cp.gain[a0 + i];
                cp.out_q[at] = cp.q_anchor[a0 + i] + L - g; cp.out_r[at] = cp.r_anchor[a0 + i] + L - g; cp.out_len[at] = g; cp.out_src[at] = i;
            }
        }
    }
}

#endif   // BA_CHAINING_UNIT == 0

template <bool BOUNDED> static hipError_t launch_fill(hipStream_t s, const ba::ChainingParams* cp) {
    const uint32_t waves = cp->ring > 1024u ? 2u : 4u;   // at most 48 KB of LDS per workgroup
    const uint32_t wgs = (cp->n + waves - 1u) / waves;
    k_chaining_fill<BOUNDED><<<dim3(wgs < 2048u ? wgs : 2048u), dim3(64u * waves), waves * 3u * cp->ring * 4u, s>>>(*cp);
    return hipGetLastError();
}
#if BA_CHAINING_UNIT == 1
extern "C" hipError_t ba_launch_chaining_fill_bounded(hipStream_t s, const ba::ChainingParams* cp) { return launch_fill<true>(s, cp); }
#else
extern "C" hipError_t ba_launch_chaining_fill(hipStream_t s, const ba::ChainingParams* cp) { return launch_fill<false>(s, cp); }
extern "C" hipError_t ba_launch_chaining_pick(hipStream_t s, const ba::ChainingParams* cp) {
    const uint32_t wgs = (cp->n + CHAINING_WAVES - 1u) / CHAINING_WAVES;
    k_chaining_pick<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * CHAINING_WAVES), 0, s>>>(*cp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_chaining_gather(hipStream_t s, const ba::ChainingParams* cp) {
    const uint32_t wgs = (cp->n + CHAINING_WAVES - 1u) / CHAINING_WAVES;
    k_chaining_gather<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * CHAINING_WAVES), 0, s>>>(*cp);
    return hipGetLastError();
}
#endif
