// block_aligner_amd — anchor-chain batches (ba_chain_batch_*): what the host (ba_host.cpp) and the segmented splice (ba_chain.hip)
// share. Plain C++, no device code.
#pragma once
#include <stdint.h>

namespace ba {

constexpr uint32_t CHAIN_NO_PIECE = 0xffffffffu;   // ChainParams::end_side / gap_side: the piece was not aligned (an empty side, a gap with an empty slice)

// The result and the CIGAR runs of one inner batch (the ends' or the gaps'), in its device order; the runs of pair d are right-aligned in
// [cig_off[d], cig_off[d + 1]). All null for a set without such pieces.
struct ChainPieces {
    const int32_t* score; const uint32_t* qidx; const uint32_t* ridx; const unsigned long long* cells;
    const uint32_t* status; const uint32_t* cig_len; const uint64_t* cig_off; const uint32_t* cig_ops;
};

// The splice (k_chain_anchors, k_chain_results, k_chain_gather): one chain = one result, in the caller's order. Chain c holds the anchors
// anchor_first[c] .. anchor_first[c + 1]; its elements are, in path order, the left end, anchor 0, gap 0, anchor 1, ..., the last anchor and
// the right end: 2 K + 1 of them for K anchors, element 0 the left end, element 2 k + 1 anchor k, element 2 k + 2 gap k, element 2 K the
// right end.
struct ChainParams {
    uint32_t n;                  // chains
    uint32_t n_anchors;
    int32_t kind;                // KIND_AA / KIND_NUC / KIND_BYTES
    uint32_t flags;              // the batch's mode bits (F_TRACE, F_CIGAR_EQ)
    int32_t gap_open, gap_extend;
    const int8_t* matrix;        // as BatchParams::matrix
    const uint64_t* anchor_first;   // n + 1
    const uint32_t* q_anchor; const uint32_t* r_anchor; const uint32_t* anchor_len;   // per anchor, oriented frame
    // per anchor, its query / reference image in anchor_pool ([NULL] + converted bytes, oriented frame)
    const uint8_t* anchor_pool; const uint64_t* anchor_q; const uint64_t* anchor_r;
    const uint32_t* end_side;    // 2 per chain: the ends batch's device position of the left / right end, or CHAIN_NO_PIECE
    const uint32_t* gap_side;    // per anchor: the gaps batch's device position of the gap behind the anchor, or CHAIN_NO_PIECE
    ChainPieces ends, gaps;
    // per anchor (k_chain_anchors): score, runs, first op | last op << 4, length of the first and of the last run
    int32_t* a_score; uint32_t* a_nrun; uint32_t* a_ops; uint32_t* a_flen; uint32_t* a_llen;
    // outputs, caller's order
    int32_t* score; int32_t* left_score; int32_t* right_score;
    uint32_t* q_start; uint32_t* r_start; uint32_t* q_end; uint32_t* r_end;
    unsigned long long* cells; uint32_t* status; uint32_t* cigar_len;
    uint64_t* out_off;           // n + 1 entries: where each chain's runs start in `runs`; out_off[n] = the total
    uint32_t* runs;              // capacity >= out_off[n]
};

}  // namespace ba
