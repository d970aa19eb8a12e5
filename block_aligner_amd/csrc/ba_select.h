// block_aligner_amd — read-level selection (ba_select_*): what the host (ba_host.cpp) and the kernels (ba_select.hip) share.
// Plain C++, no device code. The rule is stated in INTEGRATION.md, "Selecting a read's alignments".
#pragma once
#include <stdint.h>

namespace ba {

constexpr uint32_t SELECT_NONE = 0xffffffffu;      // parent and rank of an excluded candidate
constexpr uint32_t SELECT_MAX_PER_READ = 1024;     // candidates of one read: what one wave's LDS holds in k_select_mark
enum : uint8_t { SEL_PRIMARY = 0, SEL_SUPPLEMENTARY = 1, SEL_SECONDARY = 2, SEL_DROPPED = 3, SEL_EXCLUDED = 4 };

// Candidate c belongs to read[c]; the candidates of a read are neither contiguous nor ordered. strand, support, exclude and status may be
// null. status: a chain batch's BA_ST_* words; a candidate with one of the bits `failed` is excluded.
struct SelectParams {
    uint32_t n, n_reads;            // candidates, reads
    uint32_t mask_permille, sec_permille, max_secondary, mapq_max, full_support;
    int32_t min_score;
    uint32_t failed;
    const uint32_t* read; const int32_t* score; const uint32_t* q_start; const uint32_t* q_end; const uint32_t* q_len;
    const uint8_t* strand; const uint32_t* support; const uint8_t* exclude; const uint32_t* status;
    const uint32_t* order;          // the reads, the one with the most candidates first
    uint32_t* counter;              // the marking's work counter, zeroed before the launch
    // the grouping. Per candidate: its span [a, b) in the read's own frame, a = b = 0 if it is not eligible. Per read: its eligible
    // candidates, the scatter's cursor (both zeroed before the launch), the exclusive scan of the counts (n_reads + 1 entries). keys: the
    // eligible candidates grouped by read, (~biased score) << 32 | c: in arbitrary order after the scatter, in rank order after the marking.
    uint32_t* a; uint32_t* b; uint32_t* count; uint32_t* cursor; const uint64_t* first; uint64_t* keys;
    // outputs per candidate, in the caller's order
    uint8_t* cls; uint8_t* mapq; uint32_t* parent; uint32_t* rank; int32_t* sub_score;
    // outputs per read: the candidates of class <= SEL_SECONDARY, their exclusive scan (n_reads + 1 entries), and those candidates, reads in
    // order and in rank order within a read
    uint32_t* n_kept; const uint64_t* kept_first; uint32_t* kept;
};

}  // namespace ba
