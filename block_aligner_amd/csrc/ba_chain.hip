// Anchor-chain batches (ba_chain_batch_*, ba_host.cpp): the segmented splice behind the two fills. A chain's path is its left end reversed,
// anchor 0, gap 0, anchor 1, ..., its last anchor and its right end; the ends are pairs of one X-drop batch, the gaps with two non-empty
// slices pairs of one global batch, the anchors ungapped columns scored here, a gap with one empty slice a single I or D run made here.
// The fills' kernels are untouched; the anchors' images come from k_pack_images (ba_extend.hip).
//
// Runs with the same op merge at every join, and a merge can run across any number of elements (adjacent single-M anchors collapse into one
// run together with their neighbours' match runs). Per chain, one wave takes the elements 64 at a time: an element's runs less its merge
// with the element before it, summed by a wave prefix sum, give its place in the output; the length that has gathered in the run an element
// ends with, tail[e] = last_len[e] + (e is one run and merges with e - 1 ? tail[e - 1] : 0), is a segmented scan, carried from chunk to
// chunk. The run a merge group starts with is written once, by the element the group ends in, with the whole length.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

constexpr uint32_t CHAIN_WAVES = 4;   // waves per workgroup of k_chain_results and k_chain_gather: one chain per wave at a time

__device__ __forceinline__ int pair_score(int kind, const int8_t* __restrict__ m, uint32_t a, uint32_t b) {   // (as ba_extend.hip)
    if (kind == ba::KIND_NUC) return m[(a & 7) * 16 + (b & 15)];
    if (kind == ba::KIND_AA) return m[a * 32 + b];
    return a == b ? m[0] : m[1];
}
__device__ __forceinline__ uint32_t shfl(uint32_t x, uint32_t src) { return (uint32_t)__shfl((int)x, (int)src, 64); }
__device__ __forceinline__ uint64_t shfl64(uint64_t x, uint32_t src) { return (uint64_t)shfl((uint32_t)(x >> 32), src) << 32 | shfl((uint32_t)x, src); }
__device__ __forceinline__ uint32_t shfl_up(uint32_t x, int d) { return (uint32_t)__shfl_up((int)x, d, 64); }
__device__ __forceinline__ uint32_t shfl_down(uint32_t x, int d) { return (uint32_t)__shfl_down((int)x, d, 64); }
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = shfl_up(x, d);
        x += lane >= (uint32_t)d ? o : 0u;
    }
    return x;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x |= (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}

// One element of a chain as the splice sees it: its runs in path order. n = 0: the element has none (an end or a gap that is empty or was
// not aligned, anything in a batch without TRACE) and the elements around it meet.
enum : uint32_t { EL_MADE = 0, EL_ENDS = 1, EL_GAPS = 2, EL_ANCHOR = 3 };   // where the runs are: one run made here / an inner batch / the anchor's bytes
struct Elem {
    uint32_t n;             // runs
    uint32_t first, last;   // the first and the last run in path order, len << 4 | op
    uint32_t where, rev;    // EL_*; rev: the source holds the runs in reverse (the left end)
    uint64_t src;           // EL_ENDS / EL_GAPS: index of the first source run in the batch's cig_ops; EL_ANCHOR: the anchor
};
__device__ __forceinline__ Elem piece_elem(const ba::ChainPieces& pc, uint32_t d, uint32_t where, bool rev) {
    Elem x{};
    const uint32_t n = pc.cig_len[d];
    if (!n) return x;
    const uint64_t src = pc.cig_off[d + 1] - n;
    const uint32_t a = pc.cig_ops[src], b = pc.cig_ops[src + n - 1];
    x.n = n; x.src = src; x.where = where; x.rev = rev;
    x.first = rev ? b : a; x.last = rev ? a : b;
    return x;
}
// element e of chain c (anchors a0 .. a0 + K), TRACE batches
__device__ __forceinline__ Elem load_elem(const ba::ChainParams& cp, uint64_t a0, uint32_t K, uint32_t c, uint32_t e) {
    Elem x{};
    if (e == 0 || e == 2 * K) {
        const uint32_t d = cp.end_side[2 * c + (e != 0)];
        if (d != ba::CHAIN_NO_PIECE) x = piece_elem(cp.ends, d, EL_ENDS, e == 0);
    } else if (e & 1u) {
        const uint64_t a = a0 + (e - 1) / 2;
        const uint32_t ops = cp.a_ops[a];
        x.n = cp.a_nrun[a]; x.where = EL_ANCHOR; x.src = a;
        x.first = cp.a_flen[a] << 4 | (ops & 15u); x.last = cp.a_llen[a] << 4 | (ops >> 4);
    } else {
        const uint64_t a = a0 + e / 2 - 1;   // the gap behind anchor a
        const uint32_t d = cp.gap_side[a];
        if (d != ba::CHAIN_NO_PIECE) x = piece_elem(cp.gaps, d, EL_GAPS, false);
        else {
            const uint32_t L = cp.anchor_len[a];
            const uint32_t dq = cp.q_anchor[a + 1] - cp.q_anchor[a] - L, dr = cp.r_anchor[a + 1] - cp.r_anchor[a] - L;
            if (dq | dr) { x.n = 1; x.where = EL_MADE; x.first = x.last = dq ? dq << 4 | 4u : dr << 4 | 5u; }   // query bytes only: I; reference bytes only: D
        }
    }
    return x;
}

// What a lane knows about its element after the wave's scans over a chunk of 64.
struct Lane {
    Elem x;
    uint32_t m;       // the element's first run merges with the last run before it
    uint32_t mnext;   // its last run merges with the first run behind it
    uint32_t off;     // the chain's runs before the element's own (those it does not share with the elements before it)
    uint32_t tail;    // the length gathered in the run before the element's first, where m
};
// Elements base .. base + 64 of chain c. carry_off / carry_tail: runs so far / the length gathered in the last run so far, updated.
__device__ __forceinline__ Lane scan_chunk(const ba::ChainParams& cp, uint64_t a0, uint32_t K, uint32_t c, uint32_t base, uint32_t lane,
                                           uint32_t& carry_off, uint32_t& carry_tail) {
    const uint32_t nelem = 2 * K + 1, e = base + lane;
    const bool in = e < nelem;
    Lane L;
    L.x = in ? load_elem(cp, a0, K, c, e) : Elem{};
    const uint32_t lo = L.x.n ? L.x.last & 15u : 0u, fo = L.x.n ? L.x.first & 15u : 0u;   // 0: no run
    // The runs next to an element's are those of the nearest element with runs. Between two anchors lies one gap and an anchor always has
    // runs, so that element is at most two away: from the neighbouring lanes, at the chunk's edges loaded.
    uint32_t p1 = shfl_up(lo, 1), p2 = shfl_up(lo, 2), n1 = shfl_down(fo, 1), n2 = shfl_down(fo, 2);
    if (lane < 1) { p1 = 0; if (in && e >= 1) { const Elem y = load_elem(cp, a0, K, c, e - 1); p1 = y.n ? y.last & 15u : 0u; } }
    if (lane < 2) { p2 = 0; if (in && e >= 2) { const Elem y = load_elem(cp, a0, K, c, e - 2); p2 = y.n ? y.last & 15u : 0u; } }
    if (lane > 62) { n1 = 0; if (e + 1 < nelem) { const Elem y = load_elem(cp, a0, K, c, e + 1); n1 = y.n ? y.first & 15u : 0u; } }
    if (lane > 61) { n2 = 0; if (e + 2 < nelem) { const Elem y = load_elem(cp, a0, K, c, e + 2); n2 = y.n ? y.first & 15u : 0u; } }
    const uint32_t pl = p1 ? p1 : p2, nf = n1 ? n1 : n2;
    L.m = L.x.n && fo == pl;
    L.mnext = L.x.n && lo == nf;
    const uint32_t cnt = L.x.n - L.m;
    const uint32_t incl = wave_incl_sum(cnt, lane);
    L.off = carry_off + incl - cnt;
    carry_off += shfl(incl, 63);
    // tail[e] = a + (p ? tail[e - 1] : 0): an element without runs hands tail[e - 1] on, an element of one merged run adds to it, every other
    // element starts anew with its last run. (a, p) compose: an inclusive scan gives tail[e] as a function of the chunk's carry-in.
    uint32_t a = L.x.n ? L.x.last >> 4 : 0u, p = L.x.n ? (uint32_t)(L.x.n == 1 && L.m) : 1u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ao = shfl_up(a, d), po = shfl_up(p, d);
        if (lane >= (uint32_t)d) { a += p ? ao : 0u; p &= po; }
    }
    const uint32_t tail = a + (p ? carry_tail : 0u);
    const uint32_t before = shfl_up(tail, 1);
    L.tail = lane ? before : carry_tail;
    carry_tail = shfl(tail, 63);
    return L;
}

}  // namespace

// Splice, pass 1: one thread per anchor. Its score, and what the joins need of its runs (one M run; its = / X runs with CIGAR_EQ): their number,
// the first and the last op, the length of the first and of the last run.
__global__ void __launch_bounds__(256) k_chain_anchors(const ba::ChainParams cp) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= cp.n_anchors) return;
    const bool eq = cp.flags & ba::F_CIGAR_EQ;
    const uint32_t L = cp.anchor_len[a];
    const uint8_t* qs = cp.anchor_pool + cp.anchor_q[a] + 1;
    const uint8_t* rs = cp.anchor_pool + cp.anchor_r[a] + 1;
    int sc = 0;
    uint32_t nrun = 0, first_op = 0, last_op = 0, flen = 0, len = 0;
    for (uint32_t k = 0; k < L; k++) {
        const uint32_t x = qs[k], y = rs[k];
        sc += pair_score(cp.kind, cp.matrix, x, y);
        const uint32_t op = eq ? (x == y ? 2u : 3u) : 1u;
        if (op != last_op) { if (nrun == 1) flen = len; nrun++; if (!first_op) first_op = op; last_op = op; len = 0; }
        len++;
    }
    if (nrun == 1) flen = len;
    cp.a_score[a] = sc; cp.a_nrun[a] = nrun; cp.a_ops[a] = last_op << 4 | first_op; cp.a_flen[a] = flen; cp.a_llen[a] = len;
}

// Splice, pass 2: one wave per chain at a time. The sums over its elements (score, cells, the OR of the status bits), the ends' own results,
// and with TRACE the number of runs after every merge.
__global__ void __launch_bounds__(64 * CHAIN_WAVES) k_chain_results(const ba::ChainParams cp) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool trace = cp.flags & ba::F_TRACE;
    for (uint32_t c = blockIdx.x * CHAIN_WAVES + w; c < cp.n; c += gridDim.x * CHAIN_WAVES) {
        const uint64_t a0 = cp.anchor_first[c];
        const uint32_t K = (uint32_t)(cp.anchor_first[c + 1] - a0), nelem = 2 * K + 1;
        const uint32_t dl = cp.end_side[2 * c], dr = cp.end_side[2 * c + 1];
        const bool hl = dl != ba::CHAIN_NO_PIECE, hr = dr != ba::CHAIN_NO_PIECE;
        int sc = 0;
        unsigned long long cells = 0;
        uint32_t st = 0, carry_off = 0, carry_tail = 0;
        for (uint32_t base = 0; base < nelem; base += 64u) {
            const uint32_t e = base + lane;
            if (e < nelem) {
                if (e & 1u) sc += cp.a_score[a0 + (e - 1) / 2];
                else if (e == 0 || e == 2 * K) {
                    const uint32_t d = e ? dr : dl;
                    if (d != ba::CHAIN_NO_PIECE) { sc += cp.ends.score[d]; cells += cp.ends.cells[d]; st |= cp.ends.status[d]; }
                } else {
                    const uint64_t a = a0 + e / 2 - 1;
                    const uint32_t d = cp.gap_side[a];
                    if (d != ba::CHAIN_NO_PIECE) { sc += cp.gaps.score[d]; cells += cp.gaps.cells[d]; st |= cp.gaps.status[d]; }
                    else {
                        const uint32_t L = cp.anchor_len[a];
                        const uint32_t dq = cp.q_anchor[a + 1] - cp.q_anchor[a] - L, dd = dq | (cp.r_anchor[a + 1] - cp.r_anchor[a] - L);   // (one of them is 0)
                        if (dd) sc += cp.gap_open + (int)(dd - 1u) * cp.gap_extend;
                    }
                }
            }
            if (trace) (void)scan_chunk(cp, a0, K, c, base, lane, carry_off, carry_tail);
        }
        sc = (int)wave_sum((uint32_t)sc);
        const uint32_t clo = wave_sum((uint32_t)(cells & 0xffffffu)), cmid = wave_sum((uint32_t)((cells >> 24) & 0xffffffu)), chi = wave_sum((uint32_t)(cells >> 48));
        st = wave_or(st);
        if (lane == 0) {
            const uint64_t al = a0 + K - 1;
            const int ls = hl ? cp.ends.score[dl] : 0, rsc = hr ? cp.ends.score[dr] : 0;
            cp.score[c] = sc; cp.left_score[c] = ls; cp.right_score[c] = rsc;
            cp.q_start[c] = cp.q_anchor[a0] - (hl ? cp.ends.qidx[dl] : 0u);
            cp.r_start[c] = cp.r_anchor[a0] - (hl ? cp.ends.ridx[dl] : 0u);
            cp.q_end[c] = cp.q_anchor[al] + cp.anchor_len[al] + (hr ? cp.ends.qidx[dr] : 0u);
            cp.r_end[c] = cp.r_anchor[al] + cp.anchor_len[al] + (hr ? cp.ends.ridx[dr] : 0u);
            cp.cells[c] = (unsigned long long)clo + ((unsigned long long)cmid << 24) + ((unsigned long long)chi << 48);
            cp.status[c] = st;
            cp.cigar_len[c] = carry_off;
        }
    }
}

// Splice, pass 3 (TRACE): the runs of chain c at out_off[c]. One wave per chain at a time, the scans of pass 2 again. Every lane writes what its
// element starts and ends with -- the run a merge group started with gets the whole length from the element the group ends in --, an anchor's
// inner = / X runs come from the lane that holds it, and the inner runs of the ends and the aligned gaps are copied by all lanes, element by
// element, the left end's in reverse.
__global__ void __launch_bounds__(64 * CHAIN_WAVES) k_chain_gather(const ba::ChainParams cp) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x * CHAIN_WAVES + w; c < cp.n; c += gridDim.x * CHAIN_WAVES) {
        const uint64_t a0 = cp.anchor_first[c];
        const uint32_t K = (uint32_t)(cp.anchor_first[c + 1] - a0), nelem = 2 * K + 1;
        uint32_t* out = cp.runs + cp.out_off[c];
        uint32_t carry_off = 0, carry_tail = 0;
        for (uint32_t base = 0; base < nelem; base += 64u) {
            const Lane L = scan_chunk(cp, a0, K, c, base, lane, carry_off, carry_tail);
            const Elem& x = L.x;
            const uint32_t pos = L.off - L.m;   // where the element's first run is: its own place, or the run it merges into
            if (x.n) {
                if (x.n > 1 || !L.mnext) out[pos] = ((x.first >> 4) + (L.m ? L.tail : 0u)) << 4 | (x.first & 15u);   // a merge group ends in the first run
                if (x.n > 1 && !L.mnext) out[pos + x.n - 1] = x.last;
                if (x.where == EL_ANCHOR && x.n > 2) {
                    const uint32_t len_a = cp.anchor_len[x.src];
                    const uint8_t* qs = cp.anchor_pool + cp.anchor_q[x.src] + 1;
                    const uint8_t* rs = cp.anchor_pool + cp.anchor_r[x.src] + 1;
                    uint32_t op = 0, len = 0, r = 0;
                    for (uint32_t k = 0; k < len_a; k++) {
                        const uint32_t y = qs[k] == rs[k] ? 2u : 3u;
                        if (y != op && op) { if (r) out[pos + r] = len << 4 | op; r++; len = 0; }
                        op = y; len++;
                    }
                }
            }
            unsigned long long todo = __ballot((x.where == EL_ENDS || x.where == EL_GAPS) && x.n > 2);
            while (todo) {
                const uint32_t j = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1;
                const uint32_t n = shfl(x.n, j), rev = shfl(x.rev, j), at = shfl(pos, j);
                const uint64_t src = shfl64(x.src, j);
                const uint32_t* ops = shfl(x.where, j) == EL_ENDS ? cp.ends.cig_ops : cp.gaps.cig_ops;
                for (uint32_t i = 1 + lane; i + 1 < n; i += 64u) out[at + i] = ops[rev ? src + n - 1 - i : src + i];
            }
        }
    }
}

extern "C" hipError_t ba_launch_chain_results(hipStream_t s, const ba::ChainParams* cp) {
    k_chain_anchors<<<dim3((cp->n_anchors + 255) / 256), dim3(256), 0, s>>>(*cp);
    const uint32_t wgs = (cp->n + CHAIN_WAVES - 1) / CHAIN_WAVES;
    k_chain_results<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * CHAIN_WAVES), 0, s>>>(*cp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_chain_gather(hipStream_t s, const ba::ChainParams* cp) {
    const uint32_t wgs = (cp->n + CHAIN_WAVES - 1) / CHAIN_WAVES;
    k_chain_gather<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * CHAIN_WAVES), 0, s>>>(*cp);
    return hipGetLastError();
}
