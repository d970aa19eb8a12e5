// block_aligner_amd — minimizer seeding (ba_seeding_*): what the host (ba_host.cpp) and the kernels (ba_seeding.hip) share.
// Plain C++, no device code. The rule is stated in INTEGRATION.md, "Seeding".
#pragma once
#include <stdint.h>

namespace ba {

constexpr uint32_t SEEDING_MIN_K = 4, SEEDING_MAX_K = 16, SEEDING_MAX_W = 64;
constexpr uint32_t SEEDING_MAX_LEN = 0x7fffffffu - 16u;   // a sequence is shorter than this: every hit ends below 2^31
constexpr uint32_t SEEDING_SORT_LDS = 8192;               // entries of a query's sketch that k_seeding_sort sorts in LDS (64 KiB)
constexpr uint64_t SEEDING_MAX_HITS = 1ull << 28;         // the chainer's own limit

// Sequence s of a set of n problems is the query of problem s for s < n and the reference of problem s - n from there on: the offsets of
// the queries' sketches are seed_first[0 .. n], those of the references' seed_first[n .. 2n], and the queries' entries come first.
struct SeedingParams {
    uint32_t n;                      // problems
    uint32_t k, w, max_occ;
    const uint8_t* pool;             // the caller's bytes
    const uint64_t* seq_off; const uint32_t* seq_len; const uint8_t* seq_rc;   // per sequence (2n); rc: read as its reverse complement
    const uint32_t* seq_order;       // the sequences, longest first (2n)
    const uint32_t* sort_order;      // the problems, longest query first (n)
    const uint32_t* match_order;     // the problems, longest reference first (n)
    uint32_t* counter;               // the sketch's work counter, zeroed before each launch
    uint32_t* seed_cnt;              // per sequence: selected k-mers (the count pass)
    const uint64_t* seed_first;      // 2n + 1: the exclusive scan of seed_cnt
    uint32_t* seed_pos; uint32_t* seed_code;   // per selected k-mer, by sequence and within it ascending by position (the emit pass)
    uint64_t* q_key;                 // per selected k-mer of a query (seed_first[n] entries): code << 32 | pos, sorted within the problem
    uint32_t* hit_cnt;               // per problem: hits, saturating at 0xffffffff (the match's count pass)
    const uint64_t* hit_first;       // n + 1: the exclusive scan of hit_cnt
    uint32_t* q_hit; uint32_t* r_hit; uint32_t* hit_len;   // per hit, by problem and within it by (r_hit, q_hit) (the match's emit pass)
};

}  // namespace ba
