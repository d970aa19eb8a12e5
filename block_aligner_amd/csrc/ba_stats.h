// block_aligner_amd — per-alignment statistics (ba_*_stats): what the host (ba_host.cpp) and the statistics kernels (ba_stats.hip) share.
// Plain C++, no device code.
#pragma once
#include <stdint.h>

#include "ba_params.h"

namespace ba {

// One record per alignment: the layout of struct BaAlignStats (include/block_aligner_hip.h), 12 words.
struct AlignStats {
    uint32_t q_start, r_start;   // first cell of the path: the end minus what the runs consume
    uint32_t columns;            // M/=/X + I + D cells
    uint32_t matches, mismatches, positives;   // match-type columns: equal image bytes / the others / matrix score > 0
    uint32_t ins, del;           // I / D columns
    uint32_t gap_opens;          // I runs + D runs
    uint32_t longest_ins, longest_del;
    int32_t path_score;          // the runs rescored: matrix over match-type columns + open + (n - 1) extend per gap run
};
static_assert(sizeof(AlignStats) == 48, "AlignStats layout");

// status bits after which a pair's runs are not a finished path (every overflow, lost or watchdog bit): its record is all zeros.
// ST_MODE is not among them: FREE_QUERY_END_GAPS pairs that reached a down step keep their runs.
constexpr uint32_t STATS_FAILED = ST_TRACE_OVERFLOW | ST_BLOCKS_OVERFLOW | ST_CIGAR_OVERFLOW | ST_TRACEBACK_LOST | ST_WATCHDOG | ST_SLOT_TIMEOUT |
                                  ST_CLASS_OVERFLOW;

// k_stats: one wave per pair of a batch, in its device order; the record of device position d goes to out[out_pos ? out_pos[d] : d].
struct StatsParams {
    uint32_t n;
    int32_t kind;                // KIND_AA / KIND_NUC / KIND_BYTES
    int32_t gap_open, gap_extend;
    const int8_t* matrix;        // as BatchParams::matrix: AA 27x32, NUC 8x16, BYTES {match, mismatch}
    uint32_t matrix_bytes;
    // the batch's per-pair arrays (device order); pool holds [NULL] + converted bytes + padding per sequence
    const uint8_t* pool; const uint64_t* q_off; const uint32_t* q_len; const uint64_t* r_off; const uint32_t* r_len;
    const uint32_t* qidx; const uint32_t* ridx; const uint32_t* status;
    const uint32_t* cig_len; const uint64_t* cig_off; const uint32_t* cig_ops;   // runs right-aligned in [cig_off[d], cig_off[d + 1])
    const uint32_t* out_pos;     // device position -> record index; null = the same
    AlignStats* out;
};

}  // namespace ba
