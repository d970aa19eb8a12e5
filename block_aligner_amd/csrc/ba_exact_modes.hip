// Exact full-matrix scores in a batch's own mode (ba_*_exact with BA_EXACT_OWN_MODE, ba_host.cpp): the sweep of ba_exact.hip -- one wave per
// pair, bands of 64 query rows, H and the vertical-gap state handed down one lane per step, the row buffer and the per-column inputs staged
// 64 columns per access -- for BA_LOCAL_START / BA_FREE_QUERY_* batches over a sequence matrix and for sequence-to-profile batches. The
// definitions are those of include/block_aligner_hip.h ("exact scores in the batch's own mode"). A unit of its own: beside other
// instantiations the compiler generates other code for k_exact.
//
// Compiled twice, as ba_exact.hip is: plain, for the score kernels, and with BA_EXACT_TRACED for the path kernels of ba_*_exact_paths -- the
// same sweeps leaving four bits per cell (ba_exact.h), the backward walks under the mode's stop rule and through the profile's T state,
// and the join of an extension batch's two sides.
#include <hip/hip_runtime.h>

#include "ba_exact_dev.hpp"
#include "ba_launch.h"

namespace {

// ------------------------------------------------------------------ sequence matrices
// exact_pair of ba_exact.hip with the start rule as a template parameter -- row 0 and column 0, and the floor at 0 of EXACT_START_LOCAL --
// and the end rule of BA_FREE_QUERY_END_GAPS: GLOBAL then reads the maximum of the last row, which is the rmax / rj of the last band's
// last lane.
//
// TRACE: every cell leaves its nibble as exact_pair's does, trace[band][t >> 3][lane]; HV is left clear under DIAG (the walk does not read
// it there) and a BA_LOCAL_START cell with H == 0 is marked EXACT_TR_STOP. The end cell is returned for the walk. The cell update is
// written twice, under `if constexpr (!TRACE)` as it always was and traced with the ties named: the untraced kernels must keep the
// code they compile to, so a change to the recurrence goes into both bodies (here and in exact_pair_profile).
template <int KIND, int START, bool TRACE>
__device__ void exact_pair_mode(const ba::ExactParams& xp, bool end_free, const int8_t* tab, int2* rowbuf, uint32_t lane, uint32_t d, ba::Exact* out,
                                uint32_t* trace, uint2* end) {
    constexpr bool LOCAL = START == ba::EXACT_START_LOCAL, FREE0 = START != ba::EXACT_START_GLOBAL;   // FREE0: row 0 is 0 in every column
    const uint32_t ql = xp.q_len[d], rl = xp.r_len[d];
    const uint8_t* q = xp.pool + xp.q_off[d] + 1;
    const uint8_t* r = xp.pool + xp.r_off[d] + 1;
    const int go = xp.gap_open, ge = xp.gap_extend;
    const bool extend = xp.what == ba::EXACT_EXTEND, xdrop = extend && xp.x_drop >= 0;
    int best = 0; uint32_t bi = 0, bj = 0;                 // EXTEND: cell (0, 0) = 0 is the first maximum of row 0 under every start rule
    uint32_t rows = ql + 1;
    int corner = FREE0 || !rl ? 0 : go + (int)(rl - 1) * ge;   // H[|q|][|r|]; this is row 0's
    int emax = 0; uint32_t ej = 0;                         // the last row's maximum and its first column; row 0's is cell (0, 0)
    bool stopped = false;
    for (uint32_t i0 = 0; i0 < ql && !stopped; i0 += ba::EXACT_BAND) {
        const uint32_t nb = min(ba::EXACT_BAND, ql - i0);
        const bool first = i0 == 0, last = i0 + ba::EXACT_BAND >= ql;
        const uint32_t i = i0 + lane + 1;
        const bool rowok = lane < nb;
        const uint32_t qa = q_part<KIND>(rowok ? q[i - 1] : 0u);
        int Hcur = LOCAL ? 0 : go + (int)(i - 1) * ge;                  // H[i][0]
        int diag = LOCAL || i == 1 ? 0 : go + (int)(i - 2) * ge;        // H[i - 1][0]
        int Hz = NEG, Vcur = NEG;                                       // no gap ends in column 0
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
                if (first) { inH = FREE0 ? 0 : go + (int)(jc - 1) * ge; inV = NEG; }
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
                    int h = max(diag + cell_score<KIND>(tab, qa, b), max(V, Hz));
                    if constexpr (LOCAL) h = max(h, 0);
                    if (h > rmax) { rmax = h; rj = t - lane + 1; }
                    Hcur = h; Vcur = V; diag = upH;
                }
            } else {
                uint32_t bits = 0;
                if (rowok && t - lane < rl) {
                    const int V = max(upH + go, upV + ge), zext = Hz + ge;
                    Hz = max(Hcur + go, zext);
                    const int dsc = diag + cell_score<KIND>(tab, qa, b);
                    int h = max(dsc, max(V, Hz));
                    if constexpr (LOCAL) h = max(h, 0);
                    bits = (h == dsc ? ba::EXACT_TR_DIAG : (h == V ? ba::EXACT_TR_HV : 0u)) | (V == upV + ge ? ba::EXACT_TR_VEXT : 0u) |
                           (Hz == zext ? ba::EXACT_TR_ZEXT : 0u);
                    if constexpr (LOCAL) bits |= h == 0 ? ba::EXACT_TR_STOP : 0u;
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
        if (last) {
            corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
            emax = __builtin_amdgcn_readlane(rmax, (int)nb - 1); ej = (uint32_t)__builtin_amdgcn_readlane((int)rj, (int)nb - 1);
        }
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
        else if (end_free) { o.score = emax; o.query_idx = ql; o.reference_idx = ej; o.rows = ql + 1; }
        else { o.score = corner; o.query_idx = ql; o.reference_idx = rl; o.rows = ql + 1; }
        *out = o;
    }
    if constexpr (TRACE) *end = extend ? make_uint2(bi, bj) : make_uint2(ql, end_free ? ej : rl);
}

// ------------------------------------------------------------------ profiles
// One wave's slab: the pos_aa rows (32 residues, one byte each) of two chunks of 64 profile positions, a row every SLAB_ROW bytes -- nine
// dwords, so that lanes at consecutive positions read from different banks. At step t the lanes are at the 0-based columns t - 63 .. t:
// in the chunk that was staged last or in the one before, hence two.
constexpr uint32_t SLAB_ROW = 36, SLAB_BYTES = 2 * 64 * SLAB_ROW;

// The sequence-to-profile recurrence (T / Z / V / H of the header). Row 0 is not a closed form here -- a run of profile positions opens and
// closes at position-specific costs -- so it is swept as a row of its own: lane l of a band owns row i0 + l, and the row above row 0 holds
// no cell. What comes down a lane per step is T and V of the row above: V opens from T, and the diagonal's H is their maximum. The row
// buffer therefore holds {T, V}. The per-column gap costs travel like the reference bytes of the sequence form: 64 columns per load, a
// v_readlane for lane 0 and a DPP shift per step; {open_C + extend, close_C} share a register, open_R + extend has one.
//
// TRACE: the nibble of cell (i, j) is EXACT_TR_HT / TDIAG / VEXT / ZEXT at trace[i >> 6][(j - 1 + (i & 63)) >> 3][i & 63]: row 0 has a trace
// like every other row, with TDIAG never set. (Two bodies of the cell update, as in exact_pair_mode: keep them in step.)
template <bool TRACE>
__device__ void exact_pair_profile(const ba::ExactParams& xp, uint32_t max_size, int8_t* slab, int2* rowbuf, uint32_t lane, uint32_t d, ba::Exact* out,
                                   uint32_t* trace, uint2* end) {
    const uint32_t ql = xp.q_len[d], rl = xp.r_len[d];
    const uint8_t* q = xp.pool + xp.q_off[d] + 1;
    const uint8_t* img = xp.pool + xp.r_off[d];            // the AAProfile image (ba_params.h); 4-byte aligned
    const uint32_t P = ba::profile_positions(rl, max_size);
    const int16_t* goC = (const int16_t*)(img + (uint64_t)P * 96);
    const int16_t* clC = goC + P;
    const int16_t* goR = clC + P;
    const int ge = xp.gap_extend;
    const int oR0 = goR[0];
    const bool extend = xp.what == ba::EXACT_EXTEND, xdrop = extend && xp.x_drop >= 0;
    int best = NEG; uint32_t bi = 0, bj = 0;
    uint32_t rows = ql + 1;
    int corner = 0;
    bool stopped = false;
    const uint32_t nrows = ql + 1;
    for (uint32_t i0 = 0; i0 < nrows && !stopped; i0 += ba::EXACT_BAND) {
        const uint32_t nb = min(ba::EXACT_BAND, nrows - i0);
        const bool first = i0 == 0, last = i0 + ba::EXACT_BAND >= nrows;
        const uint32_t i = i0 + lane;
        const bool rowok = lane < nb;
        const uint32_t res = rowok && i ? min((uint32_t)q[i - 1], 31u) : 0u;   // (row 0 has no residue and no diagonal: its read is never the maximum)
        int Hcur = i ? oR0 + (int)i * ge : 0;                          // H[i][0]: one run of i residues before position 1
        int diag = i == 0 ? NEG : (i == 1 ? 0 : oR0 + (int)(i - 1) * ge);   // H[i - 1][0]
        int Zcur = NEG, Tcur = NEG, Vcur = NEG;                        // (column 0's T and V never come down: the sweep starts in column 1)
        int rmax = Hcur; uint32_t rj = 0;
        int inT = NEG, inV = NEG, outT = 0, outV = 0;
        int gch = 0, rch = 0, g = 0, orr = 0;
        const uint32_t T = rl ? rl + nb - 1 : 0;
        [[maybe_unused]] uint32_t acc = 0;
        [[maybe_unused]] uint32_t* tr = nullptr;
        if constexpr (TRACE) tr = trace + (uint64_t)(i0 / ba::EXACT_BAND) * ba::exact_trace_words(rl) * 64u + lane;
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t c = t & 63u;
            if (c == 0) {   // the next 64 columns: lane k holds column t + 1 + k of the row above and of the gap costs
                const uint32_t jc = t + 1 + lane;
                const bool in = jc <= rl;
                if (!first) { const int2 x = in ? rowbuf[jc] : make_int2(NEG, NEG); inT = x.x; inV = x.y; }
                gch = in ? (int)(((uint32_t)(uint16_t)(int16_t)(goC[jc] + ge)) | ((uint32_t)(uint16_t)clC[jc] << 16)) : 0;
                rch = in ? goR[jc] + ge : 0;
                // ... and their 64 x 32 scores: 512 dwords, eight per lane, dword k of the chunk belongs to position t + 1 + k / 8
                const uint32_t* src = (const uint32_t*)(img + (uint64_t)(t + 1) * 32);
                uint32_t* dst = (uint32_t*)(slab + ((t >> 6) & 1u) * (64 * SLAB_ROW));
#pragma unroll
                for (uint32_t m = 0; m < 8; m++) {
                    const uint32_t k = m * 64u + lane, col = k >> 3;
                    dst[col * (SLAB_ROW / 4) + (k & 7u)] = t + 1 + col <= rl ? src[k] : 0u;
                }
                // the other lanes' reads of this chunk follow these stores in the same wave
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            const int upT = wave_shr1_first(Tcur, __builtin_amdgcn_readlane(inT, c));
            const int upV = wave_shr1_first(Vcur, __builtin_amdgcn_readlane(inV, c));
            g = wave_shr1_first(g, __builtin_amdgcn_readlane(gch, c));
            orr = wave_shr1_first(orr, __builtin_amdgcn_readlane(rch, c));
            if constexpr (!TRACE) {
                if (rowok && t - lane < rl) {   // (unsigned: t >= lane) column j = t - lane + 1 is inside the matrix
                    const uint32_t cj = t - lane;
                    const int s = slab[(cj & 127u) * SLAB_ROW + res];
                    const int upH = max(upT, upV);
                    const int Z = max(Hcur + (int)(int16_t)(g & 0xffff), Zcur + ge);
                    const int Tn = max(diag + s, Z + (g >> 16));
                    const int V = max(upT + orr, upV + ge);
                    const int h = max(Tn, V);
                    if (h > rmax) { rmax = h; rj = cj + 1; }
                    Hcur = h; Zcur = Z; Tcur = Tn; Vcur = V; diag = upH;
                }
            } else {
                uint32_t bits = 0;
                if (rowok && t - lane < rl) {
                    const uint32_t cj = t - lane;
                    const int s = slab[(cj & 127u) * SLAB_ROW + res];
                    const int upH = max(upT, upV);
                    const int zext = Zcur + ge, vext = upV + ge;
                    const int Z = max(Hcur + (int)(int16_t)(g & 0xffff), zext);
                    const int dsc = diag + s;
                    const int Tn = max(dsc, Z + (g >> 16));
                    const int V = max(upT + orr, vext);
                    const int h = max(Tn, V);
                    bits = (h == Tn ? ba::EXACT_TR_HT : 0u) | (i != 0u && Tn == dsc ? ba::EXACT_TR_TDIAG : 0u) | (V == vext ? ba::EXACT_TR_VEXT : 0u) |
                           (Z == zext ? ba::EXACT_TR_ZEXT : 0u);
                    if (h > rmax) { rmax = h; rj = cj + 1; }
                    Hcur = h; Zcur = Z; Tcur = Tn; Vcur = V; diag = upH;
                }
                // nibble t & 7 of dword t >> 3; the band's last dword is stored short
                acc = (acc >> 4) | (bits << 28);
                if ((t & 7u) == 7u || t + 1 == T) tr[(uint64_t)(t >> 3) * 64u] = acc >> ((7u - (t & 7u)) * 4u);
            }
            if (!last) {    // lane 63's cell of this step (column t - 62) goes to slot c of the outgoing registers
                outT = lane == c ? __builtin_amdgcn_readlane(Tcur, 63) : outT;
                outV = lane == c ? __builtin_amdgcn_readlane(Vcur, 63) : outV;
                if (c == 63u || t + 1 == T) {   // slot s holds column t - c + s - 62
                    const int jo = (int)(t - c + lane) - 62;
                    if (lane <= c && jo >= 1 && jo <= (int)rl) rowbuf[jo] = make_int2(outT, outV);
                }
            }
        }
        // the next band's loads follow this band's stores in the same wave; so do the next pair's slab stores this band's slab reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
        if (extend) {
            uint32_t lim = nb;
            if (xdrop) {   // rows in order, row 0 among them: the running maximum includes the row itself
                const int run = max(best, wave_incl_max(rowok ? rmax : NEG, lane));
                const unsigned long long stop = __ballot(rowok && rmax < run - xp.x_drop);
                if (stop) {
                    const uint32_t sl = (uint32_t)__builtin_ctzll(stop);
                    lim = sl + 1; rows = i0 + sl + 1; stopped = true;
                }
            }
            const int v = lane < lim ? rmax : NEG;
            const int m = wave_max_i(v);
            if (m > best) {   // ties: the smallest row, then (rj) the smallest column
                const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(lane < lim && v == m));
                best = m; bi = i0 + l; bj = (uint32_t)__shfl((int)rj, (int)l, 64);
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

#ifdef BA_EXACT_TRACED
// ------------------------------------------------------------------ the walks
// exact_walk of ba_exact.hip -- wave-uniform position and state, two cached trace dwords per row of the current band, '=' / 'X' from cached
// image bytes, lane 0 writing the reversed, merged runs to rev[0 .. n) -- with the start rule of the batch's mode in state H (the header's
// "optimal paths in the batch's own mode"): EXACT_START_LOCAL stops at a cell marked EXACT_TR_STOP and on row 0 and column 0, where H is 0;
// EXACT_START_FREE_ROW0 stops on row 0 and emits nothing there. *start receives the cell where the walk stopped.
__device__ uint32_t exact_walk_mode(const uint32_t* trace, uint32_t tw, const uint8_t* q, const uint8_t* r, uint32_t ql, uint32_t rl, bool eq, uint32_t start_rule,
                                    uint32_t lane, uint32_t ei, uint32_t ej, uint32_t* rev, uint2* start) {
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
            if (start_rule == ba::EXACT_START_GLOBAL) { if (i == 0u) emit(5u, j); else emit(4u, i); i = 0u; j = 0u; }
            else if (start_rule == ba::EXACT_START_FREE_ROW0 && i != 0u) { emit(4u, i); i = 0u; }
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
            if (start_rule == ba::EXACT_START_LOCAL && (nib & ba::EXACT_TR_STOP) == ba::EXACT_TR_STOP) break;   // H == 0: before every move
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
    *start = make_uint2(i, j);
    return n;
}

// The profile walk: states H, V, Z and T. Row i lives in band i >> 6 (row 0 is swept); column 0 has no trace and needs none: state H ends
// there with I x i, and the only T cell of column 0 a walk reaches is (0, 0). Every match-type column is M.
// Invariant: states V, Z and T are at j >= 1, except T at (0, 0). H leaves column 0 at once; V is entered from H at j >= 1 and keeps j; T
// is entered from H or V without a move, so at j >= 1; Z is entered from T at j >= 1, and stays in Z only where ZEXT is set, which is
// never in column 1 (Z[i][0] is the sentinel), so a Z step out of column 1 lands in state H.
__device__ uint32_t exact_walk_profile(const uint32_t* trace, uint32_t tw, uint32_t lane, uint32_t ei, uint32_t ej, uint32_t* rev, uint2* start) {
    uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)ei), j = (uint32_t)__builtin_amdgcn_readfirstlane((int)ej);
    uint32_t n = 0, op = 0, len = 0, state = 0;   // state: 0 = H, 1 = V, 2 = Z, 3 = T
    uint32_t cb = ~0u, cw = 0, hi = 0, lo = 0;
    auto emit = [&](uint32_t o, uint32_t cnt) {
        if (!cnt) return;
        if (o == op) { len += cnt; return; }
        if (len) { if (lane == 0) rev[n] = (len << 4) | op; n++; }
        op = o; len = cnt;
    };
    for (;;) {
        if (j == 0u) {
            if (state == 0u) { emit(4u, i); i = 0u; break; }
            if (state == 3u) break;
        }
        const uint32_t band = i >> 6, l = i & 63u, t = j - 1u + l, w = t >> 3;
        if (band != cb || w + 1u < cw) {
            const uint32_t* p = trace + (uint64_t)band * tw * 64u + lane;
            cb = band; cw = w;
            hi = p[(uint64_t)w * 64u];
            lo = w ? p[(uint64_t)(w - 1u) * 64u] : 0u;
        }
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)(w == cw ? hi : lo), (int)l);
        const uint32_t nib = (word >> ((t & 7u) * 4u)) & 15u;
        if (state == 0u) state = (nib & ba::EXACT_TR_HT) ? 3u : 1u;
        else if (state == 3u) {
            if (nib & ba::EXACT_TR_TDIAG) { emit(1u, 1u); i--; j--; state = 0u; }
            else state = 2u;
        } else if (state == 1u) {   // (V is "no cell" in row 0: i >= 1 here)
            emit(4u, 1u);
            state = (nib & ba::EXACT_TR_VEXT) ? 1u : 3u;   // V opens from T
            i--;
        } else {
            emit(5u, 1u);
            state = (nib & ba::EXACT_TR_ZEXT) ? 2u : 0u;
            j--;
        }
    }
    if (len) { if (lane == 0) rev[n] = (len << 4) | op; n++; }
    *start = make_uint2(i, j);
    return n;
}
#endif

// the persistent loop of k_exact: a wave takes the launch's records in order through *counter
#ifndef BA_EXACT_TRACED
template <class Pair> __device__ __forceinline__ void exact_records(const ba::ExactParams& xp, uint32_t lane, Pair pair) {
    for (;;) {
        // (a convergence point, as in k_exact: lane 0's branches at the end of one pair and at the start of the next must not be threaded)
        __builtin_amdgcn_wave_barrier();
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(xp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= xp.n) break;
        const uint32_t d = xp.work[2 * k];
        ba::Exact* out = xp.out + xp.work[2 * k + 1];
        if (d == ba::EXACT_NO_PAIR) { if (lane == 0) *out = ba::Exact{}; continue; }
        pair(d, out);
    }
}
#else
// ... and of the traced kernels: pair(d, rec) also leaves record rec's run count and start cell
template <class Pair> __device__ __forceinline__ void exact_records_traced(const ba::ExactModeParams& mp, uint32_t* start_cell, uint32_t lane, Pair pair) {
    const ba::ExactParams& xp = mp.x;
    for (;;) {
        __builtin_amdgcn_wave_barrier();   // (the same convergence point)
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(xp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= xp.n) break;
        const uint32_t d = xp.work[2 * k], rec = xp.work[2 * k + 1];
        if (d == ba::EXACT_NO_PAIR) {
            if (lane == 0) { xp.out[rec] = ba::Exact{}; xp.nrun[rec] = 0u; start_cell[2 * rec] = 0u; start_cell[2 * rec + 1] = 0u; }
            continue;
        }
        pair(d, rec);
    }
}
#endif

}  // namespace

#ifndef BA_EXACT_TRACED
template <int KIND, int START>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_mode(const ba::ExactModeParams mp) {
    __shared__ int8_t tab[1024];
    const ba::ExactParams& xp = mp.x;
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = k < xp.matrix_bytes ? xp.matrix[k] : (int8_t)0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    int2* rowbuf = (int2*)xp.rows + (uint64_t)(blockIdx.x * ba::EXACT_WAVES + w) * xp.row_stride;
    const bool end_free = mp.end_free != 0;
    exact_records(xp, lane, [&](uint32_t d, ba::Exact* out) { exact_pair_mode<KIND, START, false>(xp, end_free, tab, rowbuf, lane, d, out, nullptr, nullptr); });
}

__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_profile(const ba::ExactModeParams mp) {
    __shared__ __attribute__((aligned(16))) int8_t slabs[ba::EXACT_WAVES * SLAB_BYTES];
    const ba::ExactParams& xp = mp.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    int2* rowbuf = (int2*)xp.rows + (uint64_t)(blockIdx.x * ba::EXACT_WAVES + w) * xp.row_stride;
    int8_t* slab = slabs + w * SLAB_BYTES;
    exact_records(xp, lane, [&](uint32_t d, ba::Exact* out) { exact_pair_profile<false>(xp, mp.max_size, slab, rowbuf, lane, d, out, nullptr, nullptr); });
}

template <int KIND> static void launch_mode(hipStream_t s, const ba::ExactModeParams& mp, dim3 g, dim3 b) {
    if (mp.start == ba::EXACT_START_LOCAL) k_exact_mode<KIND, ba::EXACT_START_LOCAL><<<g, b, 0, s>>>(mp);
    else if (mp.start == ba::EXACT_START_FREE_ROW0) k_exact_mode<KIND, ba::EXACT_START_FREE_ROW0><<<g, b, 0, s>>>(mp);
    else k_exact_mode<KIND, ba::EXACT_START_GLOBAL><<<g, b, 0, s>>>(mp);
}

extern "C" hipError_t ba_launch_exact_modes(hipStream_t s, const ba::ExactModeParams* mp, uint32_t wgs) {
    if (!mp->x.n || !wgs) return hipSuccess;
    const dim3 g(wgs), b(64 * ba::EXACT_WAVES);
    if (mp->x.kind == ba::KIND_PROFILE) k_exact_profile<<<g, b, 0, s>>>(*mp);
    else if (mp->x.kind == ba::KIND_NUC) launch_mode<ba::KIND_NUC>(s, *mp, g, b);
    else if (mp->x.kind == ba::KIND_AA) launch_mode<ba::KIND_AA>(s, *mp, g, b);
    else launch_mode<ba::KIND_BYTES>(s, *mp, g, b);
    return hipGetLastError();
}
#else
// The traced forms: sweep, fence, walk. A launch may run fewer than EXACT_WAVES waves per workgroup (its trace regions are cut to the free
// memory), so the wave's buffers are counted by the launch's own workgroup size.
template <int KIND, int START>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_mode_trace(const ba::ExactModeParams mp, uint32_t* start_cell) {
    __shared__ int8_t tab[1024];
    const ba::ExactParams& xp = mp.x;
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = k < xp.matrix_bytes ? xp.matrix[k] : (int8_t)0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int2* rowbuf = (int2*)xp.rows + (uint64_t)wave * xp.row_stride;
    uint32_t* trace = xp.trace + (uint64_t)wave * xp.trace_stride;
    const bool end_free = mp.end_free != 0;
    exact_records_traced(mp, start_cell, lane, [&](uint32_t d, uint32_t rec) {
        uint2 end = make_uint2(0u, 0u), start = make_uint2(0u, 0u);
        exact_pair_mode<KIND, START, true>(xp, end_free, tab, rowbuf, lane, d, xp.out + rec, trace, &end);
        // the walk's loads follow the sweep's stores in the same wave
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t nr = exact_walk_mode(trace, ba::exact_trace_words(xp.r_len[d]), xp.pool + xp.q_off[d] + 1, xp.pool + xp.r_off[d] + 1, xp.q_len[d],
                                            xp.r_len[d], xp.eq != 0, START, lane, end.x, end.y, xp.rev + xp.rev_off[rec], &start);
        if (lane == 0) { xp.nrun[rec] = nr; start_cell[2 * rec] = start.x; start_cell[2 * rec + 1] = start.y; }
    });
}

__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_profile_trace(const ba::ExactModeParams mp, uint32_t* start_cell) {
    __shared__ __attribute__((aligned(16))) int8_t slabs[ba::EXACT_WAVES * SLAB_BYTES];
    const ba::ExactParams& xp = mp.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, wave = blockIdx.x * (blockDim.x >> 6) + w;
    int2* rowbuf = (int2*)xp.rows + (uint64_t)wave * xp.row_stride;
    uint32_t* trace = xp.trace + (uint64_t)wave * xp.trace_stride;
    int8_t* slab = slabs + w * SLAB_BYTES;
    exact_records_traced(mp, start_cell, lane, [&](uint32_t d, uint32_t rec) {
        uint2 end = make_uint2(0u, 0u), start = make_uint2(0u, 0u);
        exact_pair_profile<true>(xp, mp.max_size, slab, rowbuf, lane, d, xp.out + rec, trace, &end);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t nr = exact_walk_profile(trace, ba::exact_trace_words(xp.r_len[d]), lane, end.x, end.y, xp.rev + xp.rev_off[rec], &start);
        if (lane == 0) { xp.nrun[rec] = nr; start_cell[2 * rec] = start.x; start_cell[2 * rec + 1] = start.y; }
    });
}

// Extension batches: one thread per requested seed. The left side was walked over the reversed prefixes, so its runs read backwards are
// in the order of the original sequences; then the seed's ungapped columns and the right side's runs. One run is built at a time, so
// equal ops merge across both joints (and inside the seed). Without `runs` only the count is written.
__global__ void __launch_bounds__(256) k_exact_join(const ba::ExactJoinParams jp) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= jp.m) return;
    uint32_t* dst = jp.runs ? jp.runs + jp.off[k] : nullptr;
    uint32_t n = 0, op = 0, len = 0;
    auto put = [&](uint32_t o, uint32_t cnt) {
        if (!cnt) return;
        if (o == op) { len += cnt; return; }
        if (len) { if (dst) dst[n] = (len << 4) | op; n++; }
        op = o; len = cnt;
    };
    const uint64_t l0 = jp.side_off[2 * k], r0 = jp.side_off[2 * k + 1], r1 = jp.side_off[2 * k + 2];
    for (uint64_t u = r0; u > l0; u--) { const uint32_t x = jp.side_runs[u - 1]; put(x & 15u, x >> 4); }
    const uint32_t s = jp.sel[k], L = jp.seed_len[s];
    const uint8_t* qs = jp.seed_pool + jp.seed_q[s] + 1;
    const uint8_t* rs = jp.seed_pool + jp.seed_r[s] + 1;
    if (jp.eq) for (uint32_t x = 0; x < L; x++) put(qs[x] == rs[x] ? 2u : 3u, 1u);
    else put(1u, L);
    for (uint64_t u = r0; u < r1; u++) { const uint32_t x = jp.side_runs[u]; put(x & 15u, x >> 4); }
    if (len) { if (dst) dst[n] = (len << 4) | op; n++; }
    if (!dst) jp.nrun[k] = n;
}

template <int KIND> static void launch_mode_trace(hipStream_t s, const ba::ExactModeParams& mp, uint32_t* sc, dim3 g, dim3 b) {
    if (mp.start == ba::EXACT_START_LOCAL) k_exact_mode_trace<KIND, ba::EXACT_START_LOCAL><<<g, b, 0, s>>>(mp, sc);
    else if (mp.start == ba::EXACT_START_FREE_ROW0) k_exact_mode_trace<KIND, ba::EXACT_START_FREE_ROW0><<<g, b, 0, s>>>(mp, sc);
    else k_exact_mode_trace<KIND, ba::EXACT_START_GLOBAL><<<g, b, 0, s>>>(mp, sc);
}

// `waves` waves in all, in workgroups of EXACT_WAVES (or one smaller workgroup), as ba_launch_exact_trace
extern "C" hipError_t ba_launch_exact_modes_trace(hipStream_t s, const ba::ExactModeParams* mp, uint32_t* start_cell, uint32_t waves) {
    if (!mp->x.n || !waves) return hipSuccess;
    const uint32_t per = waves < ba::EXACT_WAVES ? waves : ba::EXACT_WAVES;
    const dim3 g(waves / per), b(64 * per);
    if (mp->x.kind == ba::KIND_PROFILE) k_exact_profile_trace<<<g, b, 0, s>>>(*mp, start_cell);
    else if (mp->x.kind == ba::KIND_NUC) launch_mode_trace<ba::KIND_NUC>(s, *mp, start_cell, g, b);
    else if (mp->x.kind == ba::KIND_AA) launch_mode_trace<ba::KIND_AA>(s, *mp, start_cell, g, b);
    else launch_mode_trace<ba::KIND_BYTES>(s, *mp, start_cell, g, b);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_exact_join(hipStream_t s, const ba::ExactJoinParams* jp) {
    if (!jp->m) return hipSuccess;
    k_exact_join<<<dim3((jp->m + 255) / 256), dim3(256), 0, s>>>(*jp);
    return hipGetLastError();
}
#endif
