// The exact full-matrix DP on the device (ba_*_exact, ba_*_exact_cigars, ba_*_exact_paths; ba_host.cpp): textbook Gotoh H / E / F over the
// whole |q| x |r| matrix of a pair, in int32, from the batch's images, matrix and gaps -- under k_exact's global start rule or in the
// batch's own mode (BA_LOCAL_START / BA_FREE_QUERY_* batches, sequence-to-profile batches), scores alone or with an optimal path. No
// alignment kernel is touched; nothing of a run is read.
//
// This is the only source of the exact kernels. The Makefile compiles it into four units, -DBA_EXACT_UNIT=0 .. 3, because on this compiler
// a kernel's code depends on the instantiations that share its unit ("One source, four units"): beside the traced or the
// own-mode forms the untraced k_exact grows from 478 to 601 or 616 instructions. Bit 0 of the unit is "traced", bit 1 "own mode":
//   0  ba_exact.o              k_exact<KIND, false>, k_exact_seed
//   1  ba_exact_trace.o        k_exact<KIND, true>, k_exact_runs
//   2  ba_exact_modes.o        k_exact_mode<KIND, START>, k_exact_profile
//   3  ba_exact_modes_trace.o  k_exact_mode_trace<KIND, START>, k_exact_profile_trace, k_exact_join
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ba_exact.h"
#include "ba_launch.h"

#if !defined(BA_EXACT_UNIT) || BA_EXACT_UNIT < 0 || BA_EXACT_UNIT > 3
#error "BA_EXACT_UNIT must be 0, 1, 2 or 3"
#endif

namespace {

constexpr int NEG = ba::EXACT_NEG;

// lane l <- lane l - 1 across the whole wave; lane 0 keeps `first`
__device__ __forceinline__ int wave_shr1_first(int src, int first) { return __builtin_amdgcn_update_dpp(first, src, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int wave_max_i(int x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = max(x, __shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ int wave_incl_max(int x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(x, d, 64);
        x = lane >= (uint32_t)d ? max(x, o) : x;
    }
    return x;
}

// The fill's score of image byte a (query) against image byte b (reference), split in two: what depends on a alone (once per band and
// lane), what depends on b alone (once per 64 columns), and the table read per cell.
template <int KIND> __device__ __forceinline__ uint32_t q_part(uint32_t a) {
    if constexpr (KIND == ba::KIND_NUC) return (a & 7u) * 16u;
    else if constexpr (KIND == ba::KIND_AA) return min(a, 26u) * 32u;
    else return a;
}
template <int KIND> __device__ __forceinline__ uint32_t r_part(uint32_t b) {
    if constexpr (KIND == ba::KIND_NUC) return b & 15u;
    else if constexpr (KIND == ba::KIND_AA) return min(b, 31u);
    else return b;
}
template <int KIND> __device__ __forceinline__ int cell_score(const int8_t* tab, uint32_t qa, uint32_t rb) {
    if constexpr (KIND == ba::KIND_BYTES) return qa == rb ? tab[0] : tab[1];
    else return tab[qa + rb];
}

// ------------------------------------------------------------------ the pieces of a sweep
// One pair on one wave. Rows are query positions, columns reference positions. A band is 64 rows, one per lane; a lane walks its row left
// to right, one column per step, skewed: at step t lane l is at column t - l + 1. Two states of the row above come down one lane per step
// (DPP wave shift) -- {H, V} of a sequence matrix, {T, V} of a profile's --; the horizontal-gap state and the diagonal stay in the lane.
// Lane 0's row above is the last row of the band before, which lane 63 left in the wave's row buffer. Both ends of the buffer traffic go
// through registers 64 columns at a time (one coalesced load / store per 64 steps, a v_readlane and a select per step); the same holds
// for the per-column inputs. Every lane keeps its row's maximum and first argmax; after a band they are examined in row order.
//
// TRACE: every cell also leaves four bits for the walk (ba_exact.h, EXACT_TR_*) in the wave's trace region: trace[band][t >> 3][lane],
// nibble t & 7 (exact_trace_words), so a dword holds eight consecutive steps of one row and a store is 64 consecutive dwords.

// Lane k's entry jc = t + 1 + k of the next 64 columns of the row above.
__device__ __forceinline__ void row_above(const int2* rowbuf, uint32_t jc, bool in, int& a, int& v) {
    const int2 x = in ? rowbuf[jc] : make_int2(NEG, NEG);
    a = x.x; v = x.y;
}

// Lane 63's cell of step t (column t - 62) goes to slot c = t & 63 of the outgoing registers; they are stored when full and at the band's
// last step. Slot s holds column t - c + s - 62.
__device__ __forceinline__ void hand_over(int2* rowbuf, uint32_t lane, uint32_t t, uint32_t c, uint32_t T, uint32_t rl, int a, int v, int& outA, int& outV) {
    outA = lane == c ? __builtin_amdgcn_readlane(a, 63) : outA;
    outV = lane == c ? __builtin_amdgcn_readlane(v, 63) : outV;
    if (c == 63u || t + 1 == T) {
        const int jo = (int)(t - c + lane) - 62;
        if (lane <= c && jo >= 1 && jo <= (int)rl) rowbuf[jo] = make_int2(outA, outV);
    }
}

// A lane shifts its cell's nibble into one register per step and the wave stores that register once per eight steps: nibble t & 7 of
// dword t >> 3; the band's last dword is stored short.
__device__ __forceinline__ void trace_put(uint32_t* tr, uint32_t t, uint32_t T, uint32_t bits, uint32_t& acc) {
    acc = (acc >> 4) | (bits << 28);
    if ((t & 7u) == 7u || t + 1 == T) tr[(uint64_t)(t >> 3) * 64u] = acc >> ((7u - (t & 7u)) * 4u);
}

// The end game of an EXTEND sweep's band: lane l owns row row0 + l, nb rows in all, rmax / rj are the row's maximum and its first column.
// What the sweep carries from band to band -- the best cell so far (best at (bi, bj)), the rows that counted, and whether the X-drop rule has
// ended it -- comes as plain references: handed over as one struct, the same five values cost k_exact_mode's step loop an instruction
// ("One source, four units"). The rows are taken in order: the running maximum includes the row itself, and the first row that
// falls x_drop below it is the last one that counts.
__device__ __forceinline__ void band_end_game(int& best, uint32_t& bi, uint32_t& bj, uint32_t& rows, bool& stopped, uint32_t row0, uint32_t nb, uint32_t lane,
                                              int rmax, uint32_t rj, bool xdrop, int x_drop) {
    const bool rowok = lane < nb;
    uint32_t lim = nb;
    if (xdrop) {
        const int run = max(best, wave_incl_max(rowok ? rmax : NEG, lane));
        const unsigned long long stop = __ballot(rowok && rmax < run - x_drop);
        if (stop) {
            const uint32_t sl = (uint32_t)__builtin_ctzll(stop);
            lim = sl + 1; rows = row0 + sl + 1; stopped = true;
        }
    }
    const int v = lane < lim ? rmax : NEG;
    const int m = wave_max_i(v);
    if (m > best) {   // ties: the smallest row, then (rj) the smallest column
        const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(lane < lim && v == m));
        best = m; bi = row0 + l; bj = (uint32_t)__shfl((int)rj, (int)l, 64);
    }
}

// The pair's record, and for the walk the cell it was read from: EXTEND's best cell, or cell (|q|, gj) with score g.
template <bool TRACE>
__device__ __forceinline__ void leave_record(uint32_t lane, bool extend, int best, uint32_t bi, uint32_t bj, uint32_t rows, uint32_t ql, int g, uint32_t gj,
                                             ba::Exact* out, uint2* end) {
    if (lane == 0) {
        ba::Exact o;
        if (extend) { o.score = best; o.query_idx = bi; o.reference_idx = bj; o.rows = rows; }
        else { o.score = g; o.query_idx = ql; o.reference_idx = gj; o.rows = ql + 1; }
        *out = o;
    }
    if constexpr (TRACE) *end = extend ? make_uint2(bi, bj) : make_uint2(ql, gj);
}

// ------------------------------------------------------------------ sequence matrices
// Lane l of a band owns row i0 + l + 1; row 0 and column 0 are closed forms of the start rule (ba_exact.h, EXACT_START_*), and
// EXACT_START_LOCAL floors H at 0. end_free is the end rule of BA_FREE_QUERY_END_GAPS: GLOBAL then reads the maximum of the last row, which
// is the rmax / rj of the last band's last lane.
//
// TRACE: HV is left clear under DIAG (the walk does not read it there), and a BA_LOCAL_START cell with H == 0 is marked EXACT_TR_STOP.
template <int KIND, int START, bool TRACE>
__device__ void exact_pair(const ba::ExactParams& xp, bool end_free, const int8_t* tab, int2* rowbuf, uint32_t lane, uint32_t d, ba::Exact* out, uint32_t* trace,
                           uint2* end) {
    constexpr bool LOCAL = START == ba::EXACT_START_LOCAL, FREE0 = START != ba::EXACT_START_GLOBAL;   // FREE0: row 0 is 0 in every column
    const uint32_t ql = xp.q_len[d], rl = xp.r_len[d];
    const uint8_t* q = xp.pool + xp.q_off[d] + 1;
    const uint8_t* r = xp.pool + xp.r_off[d] + 1;
    const int go = xp.gap_open, ge = xp.gap_extend;
    const bool extend = xp.what == ba::EXACT_EXTEND, xdrop = extend && xp.x_drop >= 0;
    int best = 0; uint32_t bi = 0, bj = 0, rows = ql + 1;   // EXTEND: cell (0, 0) = 0 is the first maximum of row 0 under every start rule
    bool stopped = false;
    int corner = FREE0 || !rl ? 0 : go + (int)(rl - 1) * ge;   // H[|q|][|r|]; this is row 0's
    int emax = 0; uint32_t ej = 0;                         // the last row's maximum and its first column; row 0's is cell (0, 0)
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
                else row_above(rowbuf, jc, in, inH, inV);
                rch = r_part<KIND>(in ? r[jc - 1] : 0u);
            }
            const int upH = wave_shr1_first(Hcur, __builtin_amdgcn_readlane(inH, c));
            const int upV = wave_shr1_first(Vcur, __builtin_amdgcn_readlane(inV, c));
            b = (uint32_t)wave_shr1_first((int)b, __builtin_amdgcn_readlane((int)rch, c));
            [[maybe_unused]] uint32_t bits = 0;
            if (rowok && t - lane < rl) {   // (unsigned: t >= lane) column j = t - lane + 1 is inside the matrix
                const int V = max(upH + go, upV + ge), zext = Hz + ge;
                Hz = max(Hcur + go, zext);
                const int dsc = diag + cell_score<KIND>(tab, qa, b);
                int h = max(dsc, max(V, Hz));
                if constexpr (LOCAL) h = max(h, 0);
                if constexpr (TRACE) {
                    bits = (h == dsc ? ba::EXACT_TR_DIAG : (h == V ? ba::EXACT_TR_HV : 0u)) | (V == upV + ge ? ba::EXACT_TR_VEXT : 0u) |
                           (Hz == zext ? ba::EXACT_TR_ZEXT : 0u);
                    if constexpr (LOCAL) bits |= h == 0 ? ba::EXACT_TR_STOP : 0u;
                }
                if (h > rmax) { rmax = h; rj = t - lane + 1; }
                Hcur = h; Vcur = V; diag = upH;
            }
            if constexpr (TRACE) trace_put(tr, t, T, bits, acc);
            if (!last) hand_over(rowbuf, lane, t, c, T, rl, Hcur, Vcur, outH, outV);
        }
        // the next band's loads follow this band's stores in the same wave
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) {
            corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
            emax = __builtin_amdgcn_readlane(rmax, (int)nb - 1); ej = (uint32_t)__builtin_amdgcn_readlane((int)rj, (int)nb - 1);
        }
        if (extend) band_end_game(best, bi, bj, rows, stopped, i0 + 1, nb, lane, rmax, rj, xdrop, xp.x_drop);
    }
    leave_record<TRACE>(lane, extend, best, bi, bj, rows, ql, end_free ? emax : corner, end_free ? ej : rl, out, end);
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
// like every other row, with TDIAG never set.
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
    int best = NEG; uint32_t bi = 0, bj = 0, rows = ql + 1;   // EXTEND: row 0 is examined like every other row
    bool stopped = false;
    int corner = 0;
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
                if (!first) row_above(rowbuf, jc, in, inT, inV);
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
            [[maybe_unused]] uint32_t bits = 0;
            if (rowok && t - lane < rl) {   // (unsigned: t >= lane) column j = t - lane + 1 is inside the matrix
                const uint32_t cj = t - lane;
                const int s = slab[(cj & 127u) * SLAB_ROW + res];
                const int upH = max(upT, upV);
                const int zext = Zcur + ge, vext = upV + ge;
                const int Z = max(Hcur + (int)(int16_t)(g & 0xffff), zext);
                const int dsc = diag + s;
                const int Tn = max(dsc, Z + (g >> 16));
                const int V = max(upT + orr, vext);
                const int h = max(Tn, V);
                if constexpr (TRACE)
                    bits = (h == Tn ? ba::EXACT_TR_HT : 0u) | (i != 0u && Tn == dsc ? ba::EXACT_TR_TDIAG : 0u) | (V == vext ? ba::EXACT_TR_VEXT : 0u) |
                           (Z == zext ? ba::EXACT_TR_ZEXT : 0u);
                if (h > rmax) { rmax = h; rj = cj + 1; }
                Hcur = h; Zcur = Z; Tcur = Tn; Vcur = V; diag = upH;
            }
            if constexpr (TRACE) trace_put(tr, t, T, bits, acc);
            if (!last) hand_over(rowbuf, lane, t, c, T, rl, Tcur, Vcur, outT, outV);
        }
        // the next band's loads follow this band's stores in the same wave; so do the next pair's slab stores this band's slab reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
        if (extend) band_end_game(best, bi, bj, rows, stopped, i0, nb, lane, rmax, rj, xdrop, xp.x_drop);
    }
    leave_record<TRACE>(lane, extend, best, bi, bj, rows, ql, corner, rl, out, end);
}

// ------------------------------------------------------------------ the walks
// The optimal path of one pair, walked backwards from its end cell by the rules of include/block_aligner_hip.h ("optimal alignment paths",
// "optimal paths in the batch's own mode") over the trace the sweep has just left. The position and the state are wave-uniform.

// The walk's view of the trace: the wave keeps two dwords of every row of the current band in registers -- steps 8 cw .. 8 cw + 7 and the
// eight before, where the path goes next (a move lowers the step by one or two) -- and refills them with two coalesced loads; the cell's
// nibble is a v_readlane away.
struct TraceCursor {
    const uint32_t* trace; uint32_t tw, lane;
    uint32_t cb = ~0u, cw = 0, hi = 0, lo = 0;   // the cached band and dword index
    // the nibble of step t of the row that lane l of `band` owns
    __device__ __forceinline__ uint32_t nibble(uint32_t band, uint32_t l, uint32_t t) {
        const uint32_t w = t >> 3;
        if (band != cb || w + 1u < cw) {
            const uint32_t* p = trace + (uint64_t)band * tw * 64u + lane;
            cb = band; cw = w;
            hi = p[(uint64_t)w * 64u];
            lo = w ? p[(uint64_t)(w - 1u) * 64u] : 0u;
        }
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)(w == cw ? hi : lo), (int)l);
        return (word >> ((t & 7u) * 4u)) & 15u;
    }
};

// Runs (len << 4 | op) in the order they are put, equal neighbours merged: one run is built at a time and written to dst[n] when the op
// changes. Without `write` the runs are only counted.
struct RunEmitter {
    uint32_t* dst; bool write;
    uint32_t n = 0, op = 0, len = 0;
    __device__ __forceinline__ void flush() {
        if (!len) return;
        if (write) dst[n] = (len << 4) | op;
        n++;
    }
    __device__ __forceinline__ void put(uint32_t o, uint32_t cnt) {
        if (!cnt) return;
        if (o == op) { len += cnt; return; }
        flush();
        op = o; len = cnt;
    }
};

// A sequence matrix. With `eq` the image bytes of the band's rows and of 64 reference columns are held as the trace is, for '=' / 'X'.
// Lane 0 writes the runs, reversed and merged, to rev[0 .. n); n is returned. The start rule of the batch's mode holds in state H:
// EXACT_START_GLOBAL walks the border to (0, 0); EXACT_START_LOCAL stops at a cell marked EXACT_TR_STOP and on row 0 and column 0, where H
// is 0; EXACT_START_FREE_ROW0 stops on row 0 and emits nothing there. *start receives the cell where the walk stopped.
__device__ uint32_t exact_walk(const uint32_t* trace, uint32_t tw, const uint8_t* q, const uint8_t* r, uint32_t ql, uint32_t rl, bool eq, uint32_t start_rule,
                               uint32_t lane, uint32_t ei, uint32_t ej, uint32_t* rev, uint2* start) {
    uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)ei), j = (uint32_t)__builtin_amdgcn_readfirstlane((int)ej);
    uint32_t state = 0;                           // 0 = H, 1 = V, 2 = Z
    uint32_t qb = ~0u, qc = 0, rb = ~0u, rc = 0;  // eq: the cached band of query bytes and chunk of reference bytes
    TraceCursor cur{trace, tw, lane};
    RunEmitter runs{rev, lane == 0};
    for (;;) {
        if (state == 0u && (i == 0u || j == 0u)) {
            if (start_rule == ba::EXACT_START_GLOBAL) { if (i == 0u) runs.put(5u, j); else runs.put(4u, i); i = 0u; j = 0u; }
            else if (start_rule == ba::EXACT_START_FREE_ROW0 && i != 0u) { runs.put(4u, i); i = 0u; }
            break;
        }
        const uint32_t band = (i - 1u) >> 6, l = (i - 1u) & 63u;
        const uint32_t nib = cur.nibble(band, l, j - 1u + l);
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
                runs.put(o, 1u);
                i--; j--;
            } else state = (nib & ba::EXACT_TR_HV) ? 1u : 2u;
        } else if (state == 1u) {
            runs.put(4u, 1u);
            state = (nib & ba::EXACT_TR_VEXT) ? 1u : 0u;
            i--;
        } else {
            runs.put(5u, 1u);
            state = (nib & ba::EXACT_TR_ZEXT) ? 2u : 0u;
            j--;
        }
    }
    runs.flush();
    *start = make_uint2(i, j);
    return runs.n;
}

// A profile: states H, V, Z and T. Row i lives in band i >> 6 (row 0 is swept); column 0 has no trace and needs none: state H ends
// there with I x i, and the only T cell of column 0 a walk reaches is (0, 0). Every match-type column is M.
// Invariant: states V, Z and T are at j >= 1, except T at (0, 0). H leaves column 0 at once; V is entered from H at j >= 1 and keeps j; T
// is entered from H or V without a move, so at j >= 1; Z is entered from T at j >= 1, and stays in Z only where ZEXT is set, which is
// never in column 1 (Z[i][0] is the sentinel), so a Z step out of column 1 lands in state H.
__device__ uint32_t exact_walk_profile(const uint32_t* trace, uint32_t tw, uint32_t lane, uint32_t ei, uint32_t ej, uint32_t* rev, uint2* start) {
    uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)ei), j = (uint32_t)__builtin_amdgcn_readfirstlane((int)ej);
    uint32_t state = 0;   // 0 = H, 1 = V, 2 = Z, 3 = T
    TraceCursor cur{trace, tw, lane};
    RunEmitter runs{rev, lane == 0};
    for (;;) {
        if (j == 0u) {
            if (state == 0u) { runs.put(4u, i); i = 0u; break; }
            if (state == 3u) break;
        }
        const uint32_t nib = cur.nibble(i >> 6, i & 63u, j - 1u + (i & 63u));
        if (state == 0u) state = (nib & ba::EXACT_TR_HT) ? 3u : 1u;
        else if (state == 3u) {
            if (nib & ba::EXACT_TR_TDIAG) { runs.put(1u, 1u); i--; j--; state = 0u; }
            else state = 2u;
        } else if (state == 1u) {   // (V is "no cell" in row 0: i >= 1 here)
            runs.put(4u, 1u);
            state = (nib & ba::EXACT_TR_VEXT) ? 1u : 3u;   // V opens from T
            i--;
        } else {
            runs.put(5u, 1u);
            state = (nib & ba::EXACT_TR_ZEXT) ? 2u : 0u;
            j--;
        }
    }
    runs.flush();
    *start = make_uint2(i, j);
    return runs.n;
}

// ------------------------------------------------------------------ the kernels' bodies
// Persistent: a wave takes the launch's records in order through *counter. pair(d, rec, &start) computes record rec from pair d and, TRACE,
// returns the number of its reversed runs and the cell where its walk stopped; they go to nrun and, where the call has one, to start_cell.
template <bool TRACE, class Pair>
__device__ __forceinline__ void exact_records(const ba::ExactParams& xp, uint32_t* start_cell, uint32_t lane, Pair pair) {
    for (;;) {
        // (a convergence point: without it the compiler threads the "lane 0 writes the record" branch at the end of one pair into the
        // "lane 0 takes the next record" branch of the next, and the wave-wide operations of a pair run with lane 0 apart from the others)
        __builtin_amdgcn_wave_barrier();
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(xp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= xp.n) break;
        const uint32_t d = xp.work[2 * k], rec = xp.work[2 * k + 1];
        uint2 start = make_uint2(0u, 0u);
        uint32_t nr = 0;
        if (d == ba::EXACT_NO_PAIR) { if (lane == 0) xp.out[rec] = ba::Exact{}; }   // an all-zero record
        else nr = pair(d, rec, &start);
        if constexpr (TRACE)
            if (lane == 0) {
                xp.nrun[rec] = nr;
                if (start_cell) { start_cell[2 * rec] = start.x; start_cell[2 * rec + 1] = start.y; }
            }
    }
}

// The wave's row buffer and, TRACE, its trace region. A traced launch may run fewer than EXACT_WAVES waves per workgroup (its regions are
// cut to the free memory), so its waves are counted by the launch's own workgroup size.
template <bool TRACE> __device__ __forceinline__ void wave_regions(const ba::ExactParams& xp, int2*& rowbuf, uint32_t*& trace) {
    const uint32_t wave = blockIdx.x * (TRACE ? blockDim.x >> 6 : ba::EXACT_WAVES) + (threadIdx.x >> 6);
    rowbuf = (int2*)xp.rows + (uint64_t)wave * xp.row_stride;
    trace = TRACE ? xp.trace + (uint64_t)wave * xp.trace_stride : nullptr;
}

// Sequence batches: the matrix in LDS, then per record the sweep and, TRACE, behind a fence its walk.
template <int KIND, int START, bool TRACE>
__device__ __forceinline__ void exact_sequences(const ba::ExactParams& xp, bool end_free, uint32_t* start_cell) {
    __shared__ int8_t tab[1024];
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = k < xp.matrix_bytes ? xp.matrix[k] : (int8_t)0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    int2* rowbuf; uint32_t* trace;
    wave_regions<TRACE>(xp, rowbuf, trace);
    exact_records<TRACE>(xp, start_cell, lane, [&](uint32_t d, uint32_t rec, uint2* start) -> uint32_t {
        uint2 end = make_uint2(0u, 0u);
        exact_pair<KIND, START, TRACE>(xp, end_free, tab, rowbuf, lane, d, xp.out + rec, trace, &end);
        if constexpr (TRACE) {
            // the walk's loads follow the sweep's stores in the same wave
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            return exact_walk(trace, ba::exact_trace_words(xp.r_len[d]), xp.pool + xp.q_off[d] + 1, xp.pool + xp.r_off[d] + 1, xp.q_len[d], xp.r_len[d],
                              xp.eq != 0, START, lane, end.x, end.y, xp.rev + xp.rev_off[rec], start);
        } else return 0u;
    });
}

// ... and profile batches: a slab per wave in LDS.
template <bool TRACE> __device__ __forceinline__ void exact_profiles(const ba::ExactModeParams& mp, uint32_t* start_cell) {
    __shared__ __attribute__((aligned(16))) int8_t slabs[ba::EXACT_WAVES * SLAB_BYTES];
    const ba::ExactParams& xp = mp.x;
    const uint32_t lane = threadIdx.x & 63u;
    int8_t* slab = slabs + (threadIdx.x >> 6) * SLAB_BYTES;
    int2* rowbuf; uint32_t* trace;
    wave_regions<TRACE>(xp, rowbuf, trace);
    exact_records<TRACE>(xp, start_cell, lane, [&](uint32_t d, uint32_t rec, uint2* start) -> uint32_t {
        uint2 end = make_uint2(0u, 0u);
        exact_pair_profile<TRACE>(xp, mp.max_size, slab, rowbuf, lane, d, xp.out + rec, trace, &end);
        if constexpr (TRACE) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            return exact_walk_profile(trace, ba::exact_trace_words(xp.r_len[d]), lane, end.x, end.y, xp.rev + xp.rev_off[rec], start);
        } else return 0u;
    });
}

// host: f(KIND) with the sequence kind as a constant
template <class F> void with_kind(int32_t kind, F f) {
    if (kind == ba::KIND_NUC) f(std::integral_constant<int, ba::KIND_NUC>{});
    else if (kind == ba::KIND_AA) f(std::integral_constant<int, ba::KIND_AA>{});
    else f(std::integral_constant<int, ba::KIND_BYTES>{});
}
// ... and f(START) with the start rule
template <class F> void with_start(uint32_t start, F f) {
    if (start == ba::EXACT_START_LOCAL) f(std::integral_constant<int, ba::EXACT_START_LOCAL>{});
    else if (start == ba::EXACT_START_FREE_ROW0) f(std::integral_constant<int, ba::EXACT_START_FREE_ROW0>{});
    else f(std::integral_constant<int, ba::EXACT_START_GLOBAL>{});
}
// The launch geometry of an untraced kernel: `wgs` workgroups of EXACT_WAVES waves
void grid_of_workgroups(uint32_t wgs, dim3& g, dim3& b) { g = dim3(wgs); b = dim3(64 * ba::EXACT_WAVES); }
// ... and of a traced one: `waves` waves in all, in workgroups of EXACT_WAVES (or one smaller workgroup)
void grid_of_waves(uint32_t waves, dim3& g, dim3& b) {
    const uint32_t per = waves < ba::EXACT_WAVES ? waves : ba::EXACT_WAVES;
    g = dim3(waves / per); b = dim3(64 * per);
}

}  // namespace

// ------------------------------------------------------------------ the units
#if BA_EXACT_UNIT < 2
template <int KIND, bool TRACE>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact(const ba::ExactParams xp) {
    exact_sequences<KIND, ba::EXACT_START_GLOBAL, TRACE>(xp, false, nullptr);
}
#endif

#if BA_EXACT_UNIT == 0
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
    dim3 g, b;
    grid_of_workgroups(wgs, g, b);
    with_kind(xp->kind, [&](auto K) { k_exact<decltype(K)::value, false><<<g, b, 0, s>>>(*xp); });
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_exact_seed(hipStream_t s, const ba::ExtendParams* ep, const uint32_t* which, uint32_t m, int32_t* out) {
    if (!m) return hipSuccess;
    k_exact_seed<<<dim3((m + 255) / 256), dim3(256), 0, s>>>(*ep, which, m, out);
    return hipGetLastError();
}

#elif BA_EXACT_UNIT == 1
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

extern "C" hipError_t ba_launch_exact_trace(hipStream_t s, const ba::ExactParams* xp, uint32_t waves) {
    if (!xp->n || !waves) return hipSuccess;
    dim3 g, b;
    grid_of_waves(waves, g, b);
    with_kind(xp->kind, [&](auto K) { k_exact<decltype(K)::value, true><<<g, b, 0, s>>>(*xp); });
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

#elif BA_EXACT_UNIT == 2
template <int KIND, int START>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_mode(const ba::ExactModeParams mp) {
    exact_sequences<KIND, START, false>(mp.x, mp.end_free != 0, nullptr);
}
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_profile(const ba::ExactModeParams mp) { exact_profiles<false>(mp, nullptr); }

extern "C" hipError_t ba_launch_exact_modes(hipStream_t s, const ba::ExactModeParams* mp, uint32_t wgs) {
    if (!mp->x.n || !wgs) return hipSuccess;
    dim3 g, b;
    grid_of_workgroups(wgs, g, b);
    if (mp->x.kind == ba::KIND_PROFILE) k_exact_profile<<<g, b, 0, s>>>(*mp);
    else with_kind(mp->x.kind, [&](auto K) { with_start(mp->start, [&](auto S) { k_exact_mode<decltype(K)::value, decltype(S)::value><<<g, b, 0, s>>>(*mp); }); });
    return hipGetLastError();
}

#else
template <int KIND, int START>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_mode_trace(const ba::ExactModeParams mp, uint32_t* start_cell) {
    exact_sequences<KIND, START, true>(mp.x, mp.end_free != 0, start_cell);
}
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact_profile_trace(const ba::ExactModeParams mp, uint32_t* start_cell) {
    exact_profiles<true>(mp, start_cell);
}

// Extension batches: one thread per requested seed. The left side was walked over the reversed prefixes, so its runs read backwards are
// in the order of the original sequences; then the seed's ungapped columns and the right side's runs. One run is built at a time, so
// equal ops merge across both joints (and inside the seed). Without `runs` only the count is written.
__global__ void __launch_bounds__(256) k_exact_join(const ba::ExactJoinParams jp) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= jp.m) return;
    RunEmitter runs{jp.runs ? jp.runs + jp.off[k] : nullptr, jp.runs != nullptr};
    const uint64_t l0 = jp.side_off[2 * k], r0 = jp.side_off[2 * k + 1], r1 = jp.side_off[2 * k + 2];
    for (uint64_t u = r0; u > l0; u--) { const uint32_t x = jp.side_runs[u - 1]; runs.put(x & 15u, x >> 4); }
    const uint32_t s = jp.sel[k], L = jp.seed_len[s];
    const uint8_t* qs = jp.seed_pool + jp.seed_q[s] + 1;
    const uint8_t* rs = jp.seed_pool + jp.seed_r[s] + 1;
    if (jp.eq) for (uint32_t x = 0; x < L; x++) runs.put(qs[x] == rs[x] ? 2u : 3u, 1u);
    else runs.put(1u, L);
    for (uint64_t u = r0; u < r1; u++) { const uint32_t x = jp.side_runs[u]; runs.put(x & 15u, x >> 4); }
    runs.flush();
    if (!jp.runs) jp.nrun[k] = runs.n;
}

extern "C" hipError_t ba_launch_exact_modes_trace(hipStream_t s, const ba::ExactModeParams* mp, uint32_t* start_cell, uint32_t waves) {
    if (!mp->x.n || !waves) return hipSuccess;
    dim3 g, b;
    grid_of_waves(waves, g, b);
    if (mp->x.kind == ba::KIND_PROFILE) k_exact_profile_trace<<<g, b, 0, s>>>(*mp, start_cell);
    else
        with_kind(mp->x.kind, [&](auto K) {
            with_start(mp->start, [&](auto S) { k_exact_mode_trace<decltype(K)::value, decltype(S)::value><<<g, b, 0, s>>>(*mp, start_cell); });
        });
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_exact_join(hipStream_t s, const ba::ExactJoinParams* jp) {
    if (!jp->m) return hipSuccess;
    k_exact_join<<<dim3((jp->m + 255) / 256), dim3(256), 0, s>>>(*jp);
    return hipGetLastError();
}
#endif
