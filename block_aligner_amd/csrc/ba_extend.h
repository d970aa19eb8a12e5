// block_aligner_amd — seed-and-extend batches (ba_extend_batch_*): what the host (ba_host.cpp) and the extension kernels
// (ba_extend.hip) share. Plain C++, no device code.
#pragma once
#include <stdint.h>

namespace ba {

// How an image is cut out of the caller's raw bytes (k_pack_images): one byte per image.
enum : uint8_t {
    IMG_REVERSE = 1,      // image byte k is source byte len - 1 - k (a reversed prefix)
    IMG_COMPLEMENT = 2,   // A <-> T, C <-> G on the uppercased byte, every other letter as it is (nucleotide batches only)
};

constexpr uint32_t EXT_NO_SIDE = 0xffffffffu;   // ExtendParams::side: the side is empty and was not aligned

// The splice (k_extend_results, k_extend_offsets, k_extend_gather): one seed = one result, in the caller's order.
struct ExtendParams {
    uint32_t n;                  // seeds
    int32_t kind;                // KIND_AA / KIND_NUC / KIND_BYTES
    uint32_t flags;              // the batch's mode bits (F_TRACE, F_CIGAR_EQ)
    const int8_t* matrix;        // as BatchParams::matrix
    const uint32_t* q_seed; const uint32_t* r_seed; const uint32_t* seed_len;
    // per seed, the seed's query / reference image in seed_pool ([NULL] + converted bytes, in the seed's oriented frame)
    const uint8_t* seed_pool; const uint64_t* seed_q; const uint64_t* seed_r;
    const uint32_t* side;        // 2 per seed: the inner batch's device position of the left / right side, or EXT_NO_SIDE
    // the inner batch's per-pair arrays (device order); CIGAR runs are right-aligned in [cig_off[d], cig_off[d + 1])
    const int32_t* in_score; const uint32_t* in_qidx; const uint32_t* in_ridx; const unsigned long long* in_cells;
    const uint32_t* in_status; const uint32_t* in_cig_len; const uint64_t* in_cig_off; const uint32_t* in_cig_ops;
    // outputs, caller's order
    int32_t* score; int32_t* left_score; int32_t* right_score;
    uint32_t* q_start; uint32_t* r_start; uint32_t* q_end; uint32_t* r_end;
    unsigned long long* cells; uint32_t* status; uint32_t* cigar_len;
    uint32_t* join;              // scratch: seed runs << 2 | right join merges << 1 | left join merges
    uint64_t* out_off;           // n + 1 entries: where each seed's runs start in `runs`; out_off[n] = the total
    uint32_t* runs;              // capacity >= out_off[n]
};

}  // namespace ba
