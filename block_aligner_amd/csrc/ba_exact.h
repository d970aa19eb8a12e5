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
};

}  // namespace ba
