// block_aligner_amd — exact full-matrix scores (ba_*_exact): what the host (ba_host.cpp) and the exact kernels (ba_exact.hip) share.
// Plain C++, no device code.
#pragma once
#include <stdint.h>

#include "ba_params.h"

namespace ba {

// One record per requested pair: the layout of struct BaExact (include/block_aligner_hip.h), 4 words.
struct Exact {
    int32_t score;
    uint32_t query_idx, reference_idx;   // the cell the score was read from
    uint32_t rows;                       // query rows that counted: |q| + 1 unless the X-drop rule stopped earlier
};
static_assert(sizeof(Exact) == 16, "Exact layout");

constexpr uint32_t EXACT_GLOBAL = 0, EXACT_EXTEND = 1;
// "No cell": below every reachable score, and far enough from INT32_MIN that adding two gap costs cannot wrap.
constexpr int32_t EXACT_NEG = -(1 << 30);
// A path's score lies within (|q| + |r|) * 128 of zero (int8 substitution scores and gap costs); a pair is taken only while that stays
// above EXACT_NEG.
constexpr uint64_t EXACT_MAX_LEN2 = ((uint64_t)1 << 30) / 128 - 1;
constexpr uint32_t EXACT_BAND = 64;        // query rows per sweep: one per lane
constexpr uint32_t EXACT_WAVES = 4;        // waves per workgroup of k_exact
constexpr uint32_t EXACT_NO_PAIR = 0xffffffffu;   // ExactParams::work: no pair behind this record (an empty side); its record is all zeros

// One wave's row buffer: H and the vertical-gap state of the last row of the band above, entries 0 .. max |r| (two int32 each), padded so
// that the sweep's whole chunks of 64 columns stay inside.
BA_HD constexpr uint64_t exact_row_stride(uint32_t max_r) { return ((uint64_t)max_r + 2 * EXACT_BAND) & ~(uint64_t)(EXACT_BAND - 1); }

// The traced form (ba_*_exact_cigars): four bits per cell, what the backward walk needs to know of it.
constexpr uint32_t EXACT_TR_DIAG = 1;   // H[i][j] == H[i-1][j-1] + s(q_i, r_j)
constexpr uint32_t EXACT_TR_HV = 2;     // H[i][j] == V[i][j]; left clear under DIAG, where no walk reads it
constexpr uint32_t EXACT_TR_VEXT = 4;   // V[i][j] == V[i-1][j] + extend
constexpr uint32_t EXACT_TR_ZEXT = 8;   // Z[i][j] == Z[i][j-1] + extend
// One wave's trace region, in dwords: per band of 64 rows, one dword per lane and eight steps of the skewed sweep (|r| + 63 steps at most).
// A pair is traced while |q| * |r| <= EXACT_TRACE_MAX_CELLS; with |q| + |r| <= EXACT_MAX_LEN2 the region then stays below
// (2^31 + 70 * 2^23) / 2 bytes = 1.28 GiB.
constexpr uint64_t EXACT_TRACE_MAX_CELLS = (uint64_t)1 << 31;
BA_HD constexpr uint32_t exact_trace_words(uint32_t r_len) { return (r_len + EXACT_BAND - 1 + 7) >> 3; }
BA_HD constexpr uint64_t exact_trace_stride(uint32_t q_len, uint32_t r_len) {
    return (uint64_t)((q_len + EXACT_BAND - 1) / EXACT_BAND) * EXACT_BAND * exact_trace_words(r_len);
}

// k_exact: persistent, one wave per pair. Record k of the launch is pair work[2k] of the batch's device order and goes to out[work[2k + 1]];
// the records are sorted by |q| * |r|, largest first, and the waves take them in that order through *counter.
struct ExactParams {
    uint32_t n;                  // records of this launch
    uint32_t what;               // EXACT_GLOBAL / EXACT_EXTEND
    int32_t x_drop;              // EXTEND: < 0 = no X-drop rule
    int32_t kind;                // KIND_AA / KIND_NUC / KIND_BYTES
    int32_t gap_open, gap_extend;
    const int8_t* matrix;        // as BatchParams::matrix
    uint32_t matrix_bytes;
    // the batch's per-pair arrays (device order); pool holds [NULL] + converted bytes + padding per sequence
    const uint8_t* pool; const uint64_t* q_off; const uint32_t* q_len; const uint64_t* r_off; const uint32_t* r_len;
    const uint32_t* work;
    uint32_t* counter;           // zero before the launch
    int32_t* rows;               // per wave of the launch row_stride entries of two words: {H, vertical-gap state}
    uint64_t row_stride;
    Exact* out;
    // the traced form only: per wave trace_stride dwords of trace; record k's reversed runs go to rev + rev_off[k] (room for |q| + |r|)
    // and their number to nrun[k]; eq: match-type columns are '=' / 'X' by the image bytes
    uint32_t* trace; uint64_t trace_stride;
    uint32_t* rev; const uint64_t* rev_off; uint32_t* nrun;
    uint32_t eq;
};

// ------------------------------------------------------------------ the batch's own mode (BA_EXACT_OWN_MODE)
constexpr uint32_t EXACT_OWN_MODE = 1u << 8;   // flag bit of `what`, beside EXACT_GLOBAL / EXACT_EXTEND
// the start rule of a sequence batch: as k_exact's; H[0][j] = 0 (BA_FREE_QUERY_START_GAPS); H[0][j] = H[i][0] = 0 and H floored at 0 (BA_LOCAL_START)
constexpr uint32_t EXACT_START_GLOBAL = 0, EXACT_START_FREE_ROW0 = 1, EXACT_START_LOCAL = 2;
// A profile column adds three int8 terms to a path at most (a score or gap_extend, gap_open_C / gap_open_R, gap_close_C): a path's score
// lies within (|q| + |r|) * 384 of zero.
constexpr uint64_t EXACT_MAX_LEN2_PROFILE = ((uint64_t)1 << 30) / 384 - 1;
// k_exact_mode / k_exact_profile: ExactParams (the traced fields unused; kind may be KIND_PROFILE, r_off then names AAProfile images and
// the row buffer holds {T, vertical-gap state}) and what the mode adds.
struct ExactModeParams {
    ExactParams x;
    uint32_t start;              // EXACT_START_* (sequence kinds)
    uint32_t end_free;           // BA_FREE_QUERY_END_GAPS: EXACT_GLOBAL reads the maximum of the last row
    uint32_t max_size;           // profiles: the batch's largest block, which sizes the images (profile_positions)
};

// ------------------------------------------------------------------ optimal paths in the batch's own mode (ba_*_exact_paths).
// The traced fields of ExactParams are used as k_exact uses them; the nibble layout is exact_trace_words'. The kernels take one more
// argument, start_cell: record k's walk stopped at cell (start_cell[2k], start_cell[2k + 1]).
// Sequence kinds keep EXACT_TR_*, with one addition that costs no memory: HV is clear under DIAG, so DIAG | HV together mark "H == 0" in
// a BA_LOCAL_START matrix: the path starts here.
constexpr uint32_t EXACT_TR_STOP = EXACT_TR_DIAG | EXACT_TR_HV;
// Profiles: H == T, T == H[i-1][j-1] + s (never set in row 0), and VEXT / ZEXT as above. Row 0 is a swept row: a pair has
// ceil((|q| + 1) / 64) bands and is traced while (|q| + 1) * |r| <= EXACT_TRACE_MAX_CELLS.
constexpr uint32_t EXACT_TR_HT = 1, EXACT_TR_TDIAG = 2;
// One record of ba_*_exact_paths: the layout of struct BaExactPath, 6 words.
struct ExactPath {
    int32_t score;
    uint32_t q_start, r_start, q_end, r_end, rows;
};
static_assert(sizeof(ExactPath) == 24, "ExactPath layout");
// k_exact_join: the runs of the requested seeds of an extension batch from the traced EXTEND records of their sides (record 2k the left
// side of seed sel[k], over the reversed prefixes, record 2k + 1 the right one): the left runs turned round, the seed's ungapped columns,
// the right runs, merged. runs == nullptr: only the counts, to nrun.
struct ExactJoinParams {
    uint32_t m;                  // requested seeds
    uint32_t eq;                 // the seed's columns are '=' / 'X' by the image bytes
    const uint32_t* sel;         // their seed indices
    const uint32_t* seed_len; const uint8_t* seed_pool; const uint64_t* seed_q; const uint64_t* seed_r;
    const uint32_t* side_runs; const uint64_t* side_off;   // the sides' runs in alignment order and their 2m + 1 offsets
    uint32_t* nrun;              // m counts (first pass)
    const uint64_t* off; uint32_t* runs;   // second pass: seed k's runs go to runs + off[k]
};

}  // namespace ba
