// block_aligner_amd — the reference index (ba_ref_index_*, ba_seeding_create_indexed): what the host (ba_host.cpp) and the kernels
// (ba_index.hip, ba_index_sort.hip) share. Plain C++, no device code. The rule is stated in INTEGRATION.md, "Reference index".
#pragma once
#include <stdint.h>

namespace ba {

constexpr uint32_t INDEX_SPAN = 1024;          // windows of the reference that one work item of k_index_sketch covers (a multiple of 64)
constexpr uint32_t INDEX_MAX_PREFIX_BITS = 20; // the prefix table is over the top min(2k, 20) bits of a code
constexpr uint32_t INDEX_NO_CAP = 0xffffffffu; // max_ref_occ: no cap

// The build, of one sequence or of several ("Several sequences": no k-mer and no window holds bytes of two). The index is keys code << 32 | pos, ascending, and table[x] .. table[x + 1] bounds the keys whose code starts with the
// prefix_bits bits x (1 << prefix_bits entries and one more).
struct IndexParams {
    uint32_t k, w, len;              // the bytes of all sequences, laid end to end: the index's frame
    uint32_t n_seqs, n_spans;        // spans of INDEX_SPAN windows of one sequence, a sequence's last one shorter
    uint32_t prefix_bits;
    uint32_t n_entries;              // selected k-mers (known after the count pass)
    const uint8_t* ref;              // the bytes, on the device for the build only
    const uint64_t* seq_start;       // n_seqs + 1: where a sequence starts in the index's frame
    const uint64_t* seq_span;        // n_seqs + 1: a sequence's first span (a sequence without a k-mer has none)
    uint32_t* counter;               // the sketch's work counter, zeroed before each launch
    uint32_t* span_cnt;              // per span: selected k-mers (the count pass)
    const uint64_t* span_first;      // n_spans + 1: the exclusive scan of span_cnt
    uint64_t* unsorted;              // per selected k-mer, in position order: code << 32 | pos (the emit pass)
    const uint64_t* key;             // the same, sorted
    uint32_t* table;
    uint32_t* longest_run;           // the largest number of entries that share one code (zeroed before k_index_table)
};

// The lookup of a set of n problems -- read p on its strand against the whole reference -- and the sort of their hits. The queries'
// sketches and their sorted keys are ba::SeedingParams' (seed_first, q_key), made by ba_seeding.hip's kernels.
struct IndexLookupParams {
    uint32_t n;
    uint32_t k, max_occ, max_ref_occ;
    uint32_t prefix_bits, n_entries;
    const uint32_t* order;           // the problems, longest query first (n)
    const uint64_t* seed_first;      // n + 1: where a query's entries start
    const uint64_t* q_key;           // per selected k-mer of a query: code << 32 | pos, sorted within the problem
    const uint64_t* key;             // the index
    const uint32_t* table;
    uint32_t* hit_cnt;               // per problem: hits, saturating at 0xffffffff (the count pass)
    const uint64_t* hit_first;       // n + 1: the exclusive scan of hit_cnt
    uint64_t* hit_key;               // per hit: r_pos << 32 | q_pos (the emit pass), sorted within the problem by k_index_hit_sort
    uint32_t* q_hit; uint32_t* r_hit; uint32_t* hit_len;   // per hit, by problem and within it by (r_hit, q_hit)
};

// A canonical index ("Both strands at once"; ba_index_both.hip): IndexParams as they are, the keys code << 32 | strand << 31 | pos with
// code the smaller of a k-mer's and its reverse complement's, strand: which one that was.
constexpr uint64_t INDEX_STRAND_BIT = 1ull << 31;
constexpr uint32_t INDEX_POS_MASK = 0x7fffffffu;

// The lookup of n reads in a canonical index, each on both strands at once: read r on strand s is problem 2 r + s. lp.n, lp.order and
// lp.seed_first are per read (n, n, n + 1), lp.q_key holds the strand bit as the index's keys do, and lp.hit_cnt and lp.hit_first are per
// problem (2 n, 2 n + 1). The sort of the hits is k_index_hit_sort's, over the 2 n problems.
struct IndexBothParams {
    IndexLookupParams lp;
    const uint32_t* q_len;           // per read: its bytes (a minus-strand hit's q_hit is q_len - k - pos)
};

}  // namespace ba
