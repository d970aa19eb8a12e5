// block_aligner_amd — alignment strings (ba_*_text): what the host (ba_host.cpp) and the text kernels (ba_text.hip) share.
// Plain C++, no device code.
#pragma once
#include <stdint.h>

#include "ba_params.h"
#include "ba_stats.h"

namespace ba {

// BA_TEXT_* of include/block_aligner_hip.h: the format in the low byte, flags above it
enum : uint32_t { TEXT_CIGAR = 0, TEXT_MD = 1, TEXT_CS = 2, TEXT_FORMAT = 0xffu, TEXT_SOFT_CLIP = 1u << 8 };

// k_text_len / k_text_write: one wave per pair, pairs in device order d; pair d's text goes to the caller-order position out_pos[d]
// (null: d). A pair whose status has a STATS_FAILED bit, or that has no runs, gets empty text.
struct TextParams {
    uint32_t n;
    int32_t kind;                // KIND_AA / KIND_NUC / KIND_BYTES
    uint32_t what;               // TEXT_* format | TEXT_SOFT_CLIP
    // the sequences: batch images ([NULL] + converted bytes: skip = 1, AA images hold letter - 'A'), or -- strand != null, extension batches --
    // the caller's raw bytes (skip = 0: uppercased here, and the query reverse-complemented where strand[d] is 1, as k_pack_images does)
    const uint8_t* seq; uint32_t skip; const uint8_t* strand;
    const uint64_t* q_off; const uint32_t* q_len; const uint64_t* r_off; const uint32_t* r_len;
    const uint32_t* q_end; const uint32_t* r_end; const uint32_t* status;   // the path's end cell: its start is the end less what the runs consume
    // pair d's nrun[d] runs, in alignment order, end at ops[run_end[d + 1]]
    const uint32_t* nrun; const uint64_t* run_end; const uint32_t* ops;
    const uint32_t* out_pos;
    uint32_t* len;               // k_text_len: bytes per pair, caller order
    uint64_t* offsets;           // n + 1: the exclusive scan of len (k_text_offsets), read by k_text_write
    char* text;                  // k_text_write: capacity >= offsets[n]
};

}  // namespace ba
