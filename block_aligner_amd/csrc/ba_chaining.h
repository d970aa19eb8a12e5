// block_aligner_amd — colinear anchor chaining (ba_chaining_*): what the host (ba_host.cpp) and the kernels (ba_chaining.hip) share.
// Plain C++, no device code. The rule is stated in INTEGRATION.md, "Chaining anchors".
#pragma once
#include <stdint.h>

namespace ba {

constexpr uint32_t CHAINING_NONE = 0xffffffffu;     // pred: no predecessor; mark: the anchor is in no candidate's walk
constexpr uint32_t CHAINING_MAX_LOOKBACK = 1024;    // H
constexpr uint32_t CHAINING_MAX_CHAINS = 64;        // candidates per problem: one lane each in k_chaining_gather

// A problem p holds the anchors anchor_first[p] .. anchor_first[p + 1], sorted by (reference end, query end). pred and src are indices
// within the problem.
struct ChainingParams {
    uint32_t n;                     // problems
    int32_t match_w, drift_cost, skip_cost;
    uint32_t lookback, max_dist, bandwidth, max_chains;
    int32_t min_score;
    uint32_t min_anchors;
    uint32_t ring;                  // slots of a wave's LDS ring: a power of two >= lookback + 64
    const uint64_t* anchor_first;   // n + 1
    const uint32_t* q_anchor; const uint32_t* r_anchor; const uint32_t* anchor_len;   // per anchor
    const uint32_t* order;          // the problems, longest first
    uint32_t* counter;              // the fill's work counter, zeroed before the launch
    // per anchor. The fill: f, pred, gain. The pick: mark = the candidate (0 .. max_chains) whose walk took the anchor, pos = its place in
    // that walk counted from the chain's end.
    int32_t* f; uint32_t* pred; uint32_t* gain; uint32_t* mark; uint32_t* pos;
    // per problem and candidate (n * max_chains): anchors of the chain, 0 for a candidate that was dropped or never walked; its score
    uint32_t* cand_len; int32_t* cand_score;
    // per problem: kept chains, their anchors; the exclusive scans of both (n + 1 entries each)
    uint32_t* n_chains; uint32_t* n_kept; const uint64_t* chain_off; const uint64_t* kept_off;
    // outputs. Per kept chain, in problem order and within a problem in the order picked: its problem, rank and score and where its anchors
    // start (chain_off[n] + 1 entries); per kept anchor, in path order: the trimmed anchor and the input anchor it came from.
    uint32_t* chain_problem; uint32_t* chain_rank; int32_t* chain_score; uint64_t* out_first;
    uint32_t* out_q; uint32_t* out_r; uint32_t* out_len; uint32_t* out_src;
    // a bounded chainer ("Several sequences"): where the n_seqs sequences start in the frame of r_anchor, and where the last one ends
    // (n_seqs + 1 entries). Read by the bounded fill alone; 0 and null otherwise.
    uint32_t n_seqs; const uint64_t* seq_start;
};

}  // namespace ba
