// Exact full-matrix scores (ba_*_exact, ba_host.cpp): textbook Gotoh H / E / F over the whole |q| x |r| matrix of a pair, in int32, from
// the batch's sequence images, matrix and gaps. No alignment kernel is touched; nothing of a run is read.
#include <hip/hip_runtime.h>

#include "ba_exact_dev.hpp"
#include "ba_launch.h"

namespace {

// One pair on one wave. Rows are query positions, columns reference positions. A band is 64 rows, lane l owns row i0 + l + 1 and walks it
// left to right, one column per step, skewed: at step t lane l is at column t - l + 1. H and the vertical-gap state V of the row above
// come down one lane per step (DPP wave shift); the horizontal-gap state and the diagonal stay in the lane. Lane 0's row above is the
// last row of the band before, which lane 63 left in the wave's row buffer -- or row 0, which is computed. Both ends of the buffer
// traffic go through registers 64 columns at a time (one coalesced load / store per 64 steps, a v_readlane and a select per step); the
// same holds for the reference bytes. Every lane keeps its row's maximum and first argmax; after a band they are examined in row order.
//
// TRACE: every cell also leaves the four decisions of the walk (ba_exact.h, EXACT_TR_*) in the wave's trace region. A lane shifts its
// cell's nibble into one register per step and the wave stores that register once per eight steps, so a dword holds eight consecutive
// steps of one row and a store is 64 consecutive dwords: trace[band][t >> 3][lane], nibble t & 7 (exact_trace_words). The end cell is
// returned for the walk.
template <int KIND, bool TRACE>
__device__ void exact_pair(const ba::ExactParams& xp, const int8_t* tab, int2* rowbuf, uint32_t lane, uint32_t d, ba::Exact* out, uint32_t* trace, uint2* end) {
    const uint32_t ql = xp.q_len[d], rl = xp.r_len[d];
    const uint8_t* q = xp.pool + xp.q_off[d] + 1;
    const uint8_t* r = xp.pool + xp.r_off[d] + 1;
    const int go = xp.gap_open, ge = xp.gap_extend;
    const bool extend = xp.what == ba::EXACT_EXTEND, xdrop = extend && xp.x_drop >= 0;
    int best = 0; uint32_t bi = 0, bj = 0;                 // EXTEND: cell (0, 0) = 0 is the maximum of row 0 (gap costs are negative)
    uint32_t rows = ql + 1;
    int corner = rl ? go + (int)(rl - 1) * ge : 0;         // GLOBAL: H[|q|][|r|]; this is row 0's
    bool stopped = false;
    for (uint32_t i0 = 0; i0 < ql && !stopped; i0 += ba::EXACT_BAND) {
        const uint32_t nb = min(ba::EXACT_BAND, ql - i0);
        const bool first = i0 == 0, last = i0 + ba::EXACT_BAND >= ql;
        const uint32_t i = i0 + lane + 1;
        const bool rowok = lane < nb;
        const uint32_t qa = q_part<KIND>(rowok ? q[i - 1] : 0u);
        int Hcur = go + (int)(i - 1) * ge;                 // H[i][0]
        int diag = i == 1 ? 0 : go + (int)(i - 2) * ge;    // H[i - 1][0]
        int Hz = NEG, Vcur = NEG;                          // no gap ends in column 0
        int rmax = Hcur; uint32_t rj = 0;
        int inH = NEG, inV = NEG, outH = 0, outV = 0;
        uint32_t rch = 0, b = 0;
        const uint32_t T = rl ? rl + nb - 1 : 0;
        [[maybe_unused]] uint32_t acc = 0;
        [[maybe_unused]] uint32_t* tr = nullptr;
        if constexpr (TRACE) tr = trace + (uint64_t)(i0 / ba::EXACT_BAND) * ba::exact_trace_words(rl) * 64u + lane;
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t c = t & 63u;
            if (c == 0) {   // the next 64 columns of the row above and of the reference: lane k holds column t + 1 + k
                const uint32_t jc = t + 1 + lane;
                const bool in = jc <= rl;
                if (first) { inH = go + (int)(jc - 1) * ge; inV = NEG; }
                else { const int2 x = in ? rowbuf[jc] : make_int2(NEG, NEG); inH = x.x; inV = x.y; }
                rch = r_part<KIND>(in ? r[jc - 1] : 0u);
            }
            const int upH = wave_shr1_first(Hcur, __builtin_amdgcn_readlane(inH, c));
            const int upV = wave_shr1_first(Vcur, __builtin_amdgcn_readlane(inV, c));
            b = (uint32_t)wave_shr1_first((int)b, __builtin_amdgcn_readlane((int)rch, c));
            if constexpr (!TRACE) {
                if (rowok && t - lane < rl) {   // (unsigned: t >= lane) column j = t - lane + 1 is inside the matrix
                    const int V = max(upH + go, upV + ge);
                    Hz = max(Hcur + go, Hz + ge);
                    const int h = max(diag + cell_score<KIND>(tab, qa, b), max(V, Hz));
                    if (h > rmax) { rmax = h; rj = t - lane + 1; }
                    Hcur = h; Vcur = V; diag = upH;
                }
            } else {
                uint32_t bits = 0;
                if (rowok && t - lane < rl) {
                    const int V = max(upH + go, upV + ge), zext = Hz + ge;
                    Hz = max(Hcur + go, zext);
                    const int dsc = diag + cell_score<KIND>(tab, qa, b);
                    const int h = max(dsc, max(V, Hz));
                    bits = (h == dsc ? ba::EXACT_TR_DIAG : 0u) | (h == V ? ba::EXACT_TR_HV : 0u) | (V == upV + ge ? ba::EXACT_TR_VEXT : 0u) |
                           (Hz == zext ? ba::EXACT_TR_ZEXT : 0u);
                    if (h > rmax) { rmax = h; rj = t - lane + 1; }
                    Hcur = h; Vcur = V; diag = upH;
                }
                // nibble t & 7 of dword t >> 3; the band's last dword is stored short
                acc = (acc >> 4) | (bits << 28);
                if ((t & 7u) == 7u || t + 1 == T) tr[(uint64_t)(t >> 3) * 64u] = acc >> ((7u - (t & 7u)) * 4u);
            }
            if (!last) {    // lane 63's cell of this step (column t - 62) goes to slot c of the outgoing registers
                outH = lane == c ? __builtin_amdgcn_readlane(Hcur, 63) : outH;
                outV = lane == c ? __builtin_amdgcn_readlane(Vcur, 63) : outV;
                if (c == 63u || t + 1 == T) {   // slot s holds column t - c + s - 62
                    const int jo = (int)(t - c + lane) - 62;
                    if (lane <= c && jo >= 1 && jo <= (int)rl) rowbuf[jo] = make_int2(outH, outV);
                }
            }
        }
        // the next band's loads follow this band's stores in the same wave
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
        if (extend) {
            uint32_t lim = nb;
            if (xdrop) {   // rows in order: the running maximum includes the row itself; the first row that falls x_drop below it is the last one
                const int run = max(best, wave_incl_max(rowok ? rmax : NEG, lane));
                const unsigned long long stop = __ballot(rowok && rmax < run - xp.x_drop);
                if (stop) {
                    const uint32_t sl = (uint32_t)__builtin_ctzll(stop);
                    lim = sl + 1; rows = i0 + sl + 2; stopped = true;
                }
            }
            const int v = lane < lim ? rmax : NEG;
            const int m = wave_max_i(v);
            if (m > best) {   // ties: the smallest row, then (rj) the smallest column
                const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(lane < lim && v == m));
                best = m; bi = i0 + l + 1; bj = (uint32_t)__shfl((int)rj, (int)l, 64);
            }
        }
    }
    if (lane == 0) {
        ba::Exact o;
        if (extend) { o.score = best; o.query_idx = bi; o.reference_idx = bj; o.rows = rows; }
        else { o.score = corner; o.query_idx = ql; o.reference_idx = rl; o.rows = ql + 1; }
        *out = o;
    }
    if constexpr (TRACE) *end = extend ? make_uint2(bi, bj) : make_uint2(ql, rl);
}

// The optimal path of one pair, walked backwards from its end cell (ei, ej) by the rule of include/block_aligner_hip.h ("optimal
// alignment paths") over the trace the sweep has just left. The position and the state are wave-uniform. The wave keeps two dwords of
// every row of the current band in registers -- steps 8 cw .. 8 cw + 7 and the eight before, where the path goes next (a move lowers the step by one
// or two) -- and refills them with two coalesced loads; the cell's nibble is a v_readlane away. With `eq` the image bytes of the band's
// rows and of 64 reference columns are held the same way. Lane 0 writes a run when the op changes: the runs arrive reversed and merged
// in rev[0 .. n), n is returned.
__device__ uint32_t exact_walk(const uint32_t* trace, uint32_t tw, const uint8_t* q, const uint8_t* r, uint32_t ql, uint32_t rl, bool eq, uint32_t lane,
                               uint32_t ei, uint32_t ej, uint32_t* rev) {
    uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)ei), j = (uint32_t)__builtin_amdgcn_readfirstlane((int)ej);
    uint32_t n = 0, op = 0, len = 0, state = 0;   // state: 0 = H, 1 = V, 2 = Z
    uint32_t cb = ~0u, cw = 0, hi = 0, lo = 0;    // the cached band and dword index
    uint32_t qb = ~0u, qc = 0, rb = ~0u, rc = 0;  // eq: the cached band of query bytes and chunk of reference bytes
    auto emit = [&](uint32_t o, uint32_t cnt) {
        if (!cnt) return;
        if (o == op) { len += cnt; return; }
        if (len) { if (lane == 0) rev[n] = (len << 4) | op; n++; }
        op = o; len = cnt;
    };
    for (;;) {
        if (state == 0u && (i == 0u || j == 0u)) {
            if (i == 0u) emit(5u, j); else emit(4u, i);
            break;
        }
        const uint32_t band = (i - 1u) >> 6, l = (i - 1u) & 63u, t = j - 1u + l, w = t >> 3;
        if (band != cb || w + 1u < cw) {
            const uint32_t* p = trace + (uint64_t)band * tw * 64u + lane;
            cb = band; cw = w;
            hi = p[(uint64_t)w * 64u];
            lo = w ? p[(uint64_t)(w - 1u) * 64u] : 0u;
        }
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)(w == cw ? hi : lo), (int)l);
        const uint32_t nib = (word >> ((t & 7u) * 4u)) & 15u;
        if (state == 0u) {
            if (nib & ba::EXACT_TR_DIAG) {
                uint32_t o = 1u;
                if (eq) {
                    if (band != qb) { qb = band; qc = band * 64u + lane < ql ? q[band * 64u + lane] : 0u; }
                    const uint32_t ch = (j - 1u) >> 6;
                    if (ch != rb) { rb = ch; rc = ch * 64u + lane < rl ? r[ch * 64u + lane] : 0u; }
                    o = __builtin_amdgcn_readlane((int)qc, (int)l) == __builtin_amdgcn_readlane((int)rc, (int)((j - 1u) & 63u)) ? 2u : 3u;
                }
                emit(o, 1u);
                i--; j--;
            } else state = (nib & ba::EXACT_TR_HV) ? 1u : 2u;
        } else if (state == 1u) {
            emit(4u, 1u);
            state = (nib & ba::EXACT_TR_VEXT) ? 1u : 0u;
            i--;
        } else {
            emit(5u, 1u);
            state = (nib & ba::EXACT_TR_ZEXT) ? 2u : 0u;
            j--;
        }
    }
    if (len) { if (lane == 0) rev[n] = (len << 4) | op; n++; }
    return n;
}

}  // namespace

template <int KIND, bool TRACE>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact(const ba::ExactParams xp) {
    __shared__ int8_t tab[1024];
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = k < xp.matrix_bytes ? xp.matrix[k] : (int8_t)0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    // (a traced launch may have to run fewer than EXACT_WAVES waves per workgroup: its regions are cut to the free memory)
    int2* rowbuf = (int2*)xp.rows + (uint64_t)(blockIdx.x * ba::EXACT_WAVES + w) * xp.row_stride;
    uint32_t* trace = nullptr;
    if constexpr (TRACE) {
        const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + w;
        rowbuf = (int2*)xp.rows + (uint64_t)wave * xp.row_stride;
        trace = xp.trace + (uint64_t)wave * xp.trace_stride;
    }
    for (;;) {
        // (a convergence point: without it the compiler threads the "lane 0 writes the record" branch at the end of one pair into the
        // "lane 0 takes the next record" branch of the next, and the wave-wide operations below run with lane 0 apart from the others)
        __builtin_amdgcn_wave_barrier();
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(xp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= xp.n) break;
        const uint32_t d = xp.work[2 * k];
        ba::Exact* out = xp.out + xp.work[2 * k + 1];
        if constexpr (TRACE) if (d == ba::EXACT_NO_PAIR && lane == 0) xp.nrun[xp.work[2 * k + 1]] = 0u;
        if (d == ba::EXACT_NO_PAIR) { if (lane == 0) *out = ba::Exact{}; continue; }
        uint2 end = make_uint2(0u, 0u);
        exact_pair<KIND, TRACE>(xp, tab, rowbuf, lane, d, out, trace, &end);
        if constexpr (TRACE) {
            // the walk's loads follow the sweep's stores in the same wave
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const uint32_t rec = xp.work[2 * k + 1];
            const uint32_t nr = exact_walk(trace, ba::exact_trace_words(xp.r_len[d]), xp.pool + xp.q_off[d] + 1, xp.pool + xp.r_off[d] + 1, xp.q_len[d],
                                           xp.r_len[d], xp.eq != 0, lane, end.x, end.y, xp.rev + xp.rev_off[rec]);
            if (lane == 0) xp.nrun[rec] = nr;
        }
    }
}

// This file is compiled twice: plain, for the untraced kernels and the seed scores, and with BA_EXACT_TRACED for the traced kernels and the
// run gather. (In one unit the traced instantiations change the code the compiler generates for the untraced ones.)
#ifndef BA_EXACT_TRACED
// Extension batches: the score of every requested seed's ungapped columns (read from seed_pool, as the splice reads them); one thread per
// record.
__global__ void __launch_bounds__(256) k_exact_seed(const ba::ExtendParams ep, const uint32_t* __restrict__ which, uint32_t m, int32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t s = which[k];
    const uint32_t L = ep.seed_len[s];
    const uint8_t* qs = ep.seed_pool + ep.seed_q[s] + 1;
    const uint8_t* rs = ep.seed_pool + ep.seed_r[s] + 1;
    int sc = 0;
    for (uint32_t x = 0; x < L; x++) {
        const uint32_t a = qs[x], b = rs[x];
        if (ep.kind == ba::KIND_NUC) sc += ep.matrix[(a & 7u) * 16u + (b & 15u)];
        else if (ep.kind == ba::KIND_AA) sc += ep.matrix[min(a, 26u) * 32u + min(b, 31u)];
        else sc += a == b ? ep.matrix[0] : ep.matrix[1];
    }
    out[k] = sc;
}

extern "C" hipError_t ba_launch_exact(hipStream_t s, const ba::ExactParams* xp, uint32_t wgs) {
    if (!xp->n || !wgs) return hipSuccess;
    const dim3 g(wgs), b(64 * ba::EXACT_WAVES);
    if (xp->kind == ba::KIND_NUC) k_exact<ba::KIND_NUC, false><<<g, b, 0, s>>>(*xp);
    else if (xp->kind == ba::KIND_AA) k_exact<ba::KIND_AA, false><<<g, b, 0, s>>>(*xp);
    else k_exact<ba::KIND_BYTES, false><<<g, b, 0, s>>>(*xp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_exact_seed(hipStream_t s, const ba::ExtendParams* ep, const uint32_t* which, uint32_t m, int32_t* out) {
    if (!m) return hipSuccess;
    k_exact_seed<<<dim3((m + 255) / 256), dim3(256), 0, s>>>(*ep, which, m, out);
    return hipGetLastError();
}
#else
// The reversed runs of every record, turned round into the contiguous run array at the record's offset; one wave per record.
__global__ void __launch_bounds__(256) k_exact_runs(const uint32_t* __restrict__ rev, const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ nrun,
                                                    const uint64_t* __restrict__ off, uint32_t* __restrict__ runs, uint32_t m) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6); k < m; k += gridDim.x * 4u) {
        const uint32_t n = nrun[k];
        const uint32_t* src = rev + rev_off[k];
        uint32_t* dst = runs + off[k];
        for (uint32_t u = lane; u < n; u += 64u) dst[u] = src[n - 1u - u];
    }
}

// the traced form: `waves` waves in all, in workgroups of EXACT_WAVES (or one smaller workgroup)
extern "C" hipError_t ba_launch_exact_trace(hipStream_t s, const ba::ExactParams* xp, uint32_t waves) {
    if (!xp->n || !waves) return hipSuccess;
    const uint32_t per = waves < ba::EXACT_WAVES ? waves : ba::EXACT_WAVES;
    const dim3 g(waves / per), b(64 * per);
    if (xp->kind == ba::KIND_NUC) k_exact<ba::KIND_NUC, true><<<g, b, 0, s>>>(*xp);
    else if (xp->kind == ba::KIND_AA) k_exact<ba::KIND_AA, true><<<g, b, 0, s>>>(*xp);
    else k_exact<ba::KIND_BYTES, true><<<g, b, 0, s>>>(*xp);
    return hipGetLastError();
}
// nrun (m records) -> runs at off (the offsets are ba_launch_offsets' of nrun)
extern "C" hipError_t ba_launch_exact_runs(hipStream_t s, const uint32_t* rev, const uint64_t* rev_off, const uint32_t* nrun, const uint64_t* off, uint32_t* runs,
                                           uint32_t m) {
    if (!m) return hipSuccess;
    const uint32_t wgs = (m + 3u) / 4u;
    k_exact_runs<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(256), 0, s>>>(rev, rev_off, nrun, off, runs, m);
    return hipGetLastError();
}
#endif
