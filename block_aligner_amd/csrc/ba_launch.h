// block_aligner_amd — what the host (ba_host.cpp) and the kernel translation units share about launching: the catalogue of the
// alignment kernels and the prototypes of every other launcher. Both sides include it, so the compiler checks each signature.
#pragma once
#include <hip/hip_runtime_api.h>

#include "ba_chain.h"
#include "ba_chaining.h"
#include "ba_exact.h"
#include "ba_extend.h"
#include "ba_index.h"
#include "ba_params.h"
#include "ba_seeding.h"
#include "ba_select.h"
#include "ba_stats.h"
#include "ba_text.h"

namespace ba {

// The kernel families as the host thinks of them (ba_host.cpp family_of).
enum KernelFamily {
    FAM_PAIR,        // k_align: one pair per wave, block classes 128 .. 2048 cells
    FAM_TILED,       // k_align's row-tiled class: blocks of 4096 .. 32768 cells
    FAM_MULTI,       // k_multi: four slots of 128 cells per wave
    FAM_MULTI_256,   // ... two slots of 256 cells
    FAM_MULTI_512,   // ... one slot of 512 cells
    FAM_MULTI_G2,    // ... four slots of 128 cells in four-wave workgroups at two waves per SIMD
    FAM_MULTI_G3,    // ... at three
    FAM_SMALL,       // k_small: sixteen slots of 32 cells per wave
    FAM_QUAD,        // k_quad: four pairs per wave while their block is 32 cells
    FAM_COUNT
};
constexpr int N_KINDS = 4, N_CLASSES = 6;   // block classes: 128 << c cells for c = 0 .. 4; 5 = row-tiled

// One family as one translation unit instantiates it. fn[form][trace][xdrop] are the kernels' host addresses, each taking one
// BatchParams by value. A family has one form -- except k_multi and k_small in a special-mode unit: form 0 is for LOCAL_START
// batches, form 1 for FREE_QUERY_START_GAPS batches. fn64[form][xdrop]: k_multi's traced kernels for batches whose sequence pool does not
// fit in 32 bits (F_POOL64, k_multi_p64 of ba_multi.hpp); null in every other family, whose kernels take any pool.
struct KernelEntry {
    KernelFamily family;
    unsigned wpw;   // waves per workgroup the kernels are launched with
    unsigned lds;   // bytes of LDS per workgroup where the kernel fixes them (k_quad); 0: the host sizes them by the block class
    const void* fn[2][2][2];
    const void* fn64[2][2];
};

// A kernel translation unit (ba_kernels.hip, compiled per matrix kind, packed registers per lane = 1 .. 16 or 32 for the
// row-tiled class, plain / special modes) hands over its entries while the library loads; returns their number.
int register_kernels(int kind, int pmax, bool special, const KernelEntry* entries, int n);

}  // namespace ba

// ------------------------------------------------------------------ launchers of the kernels that exist once
extern "C" {
// ba_kernels.hip
hipError_t ba_launch_traceback(hipStream_t s, const ba::BatchParams* bp);
hipError_t ba_launch_lane_kat(hipStream_t s, int form, const short* x, short* out, int gap_extend, unsigned waves);
hipError_t ba_launch_prim_kat(hipStream_t s, int op, const int* x, int* out, unsigned long long k, unsigned waves);
hipError_t ba_launch_sort_kat(hipStream_t s, int threads, uint64_t* keys, uint32_t n, uint32_t* lb);
hipError_t ba_launch_walk(hipStream_t s, const ba::BatchParams* bp, uint32_t grid);
hipError_t ba_launch_walk_l2(hipStream_t s, const ba::BatchParams* bp, uint32_t grid);
hipError_t ba_launch_walk_loc(hipStream_t s, const ba::BatchParams* bp, uint32_t grid);
hipError_t ba_launch_merge_retry(hipStream_t s, const uint32_t* idx, uint32_t k, const ba::BatchParams* sub, const ba::BatchParams* dst,
                                 const uint32_t* sub_tw, uint32_t* dst_tw);
hipError_t ba_launch_compact_cigars(hipStream_t s, const uint32_t* ops, const uint64_t* cig_off, const uint32_t* cig_len,
                                    const uint64_t* out_off, uint32_t* out, uint32_t n);
hipError_t ba_launch_cigar_offsets_and_compact(hipStream_t s, const uint32_t* ops, const uint64_t* cig_off, const uint32_t* cig_len, const uint32_t* dev_of,
                                               uint64_t* out_off, uint32_t* out, unsigned long long* total, unsigned long long capacity, uint32_t n);
hipError_t ba_launch_pack_sequences(hipStream_t s, int kind, const uint8_t* raw, const uint64_t* raw_q, const uint64_t* raw_r,
                                    const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                    uint8_t* image, uint32_t pad, uint32_t n, unsigned long long* err);
// ba_extend.hip
hipError_t ba_launch_pack_images(hipStream_t s, int kind, const uint8_t* raw, const uint64_t* raw_q, const uint64_t* raw_r, const uint8_t* flags,
                                 const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                 uint8_t* image, uint32_t pad, uint32_t n, unsigned long long* err);
hipError_t ba_launch_extend_results(hipStream_t s, const ba::ExtendParams* ep);
hipError_t ba_launch_extend_gather(hipStream_t s, const ba::ExtendParams* ep);
// ba_chain.hip
hipError_t ba_launch_chain_results(hipStream_t s, const ba::ChainParams* cp);
hipError_t ba_launch_chain_gather(hipStream_t s, const ba::ChainParams* cp);
// ba_chaining.hip (the bounded fill: its unit BA_CHAINING_UNIT 1)
hipError_t ba_launch_chaining_fill(hipStream_t s, const ba::ChainingParams* cp);
hipError_t ba_launch_chaining_fill_bounded(hipStream_t s, const ba::ChainingParams* cp);
hipError_t ba_launch_chaining_pick(hipStream_t s, const ba::ChainingParams* cp);
hipError_t ba_launch_chaining_gather(hipStream_t s, const ba::ChainingParams* cp);
// ba_seeding.hip (emit 0: the count pass, 1: the emit pass)
hipError_t ba_launch_seeding_sketch(hipStream_t s, const ba::SeedingParams* sp, int emit);
hipError_t ba_launch_seeding_sort(hipStream_t s, const ba::SeedingParams* sp);
hipError_t ba_launch_seeding_match(hipStream_t s, const ba::SeedingParams* sp, int emit);
// ba_index.hip (emit 0: the count pass, 1: the emit pass) and ba_index_sort.hip (temp null: only *temp_bytes is set)
hipError_t ba_launch_index_sketch(hipStream_t s, const ba::IndexParams* ip, int emit);
hipError_t ba_launch_index_table(hipStream_t s, const ba::IndexParams* ip);
hipError_t ba_launch_index_lookup(hipStream_t s, const ba::IndexLookupParams* lp, int emit);
hipError_t ba_launch_index_hit_sort(hipStream_t s, const ba::IndexLookupParams* lp);
hipError_t ba_launch_index_sort(hipStream_t s, const uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits, void* temp, size_t* temp_bytes);
// ba_index_both.hip: a canonical index's sketch, and the sketch and the lookup of reads taken on both strands at once
hipError_t ba_launch_both_index_sketch(hipStream_t s, const ba::IndexParams* ip, int emit);
hipError_t ba_launch_both_read_sketch(hipStream_t s, const ba::SeedingParams* sp, int emit);
hipError_t ba_launch_both_lookup(hipStream_t s, const ba::IndexBothParams* bp, int emit);
// ba_select.hip (scatter 0: the count pass, 1: the scatter pass)
hipError_t ba_launch_select_group(hipStream_t s, const ba::SelectParams* sp, int scatter);
hipError_t ba_launch_select_mark(hipStream_t s, const ba::SelectParams* sp);
hipError_t ba_launch_select_emit(hipStream_t s, const ba::SelectParams* sp);
// ba_stats.hip
hipError_t ba_launch_stats(hipStream_t s, const ba::StatsParams* sp);
hipError_t ba_launch_stats_extend(hipStream_t s, const ba::ExtendParams* ep, const ba::AlignStats* side, ba::AlignStats* out);
hipError_t ba_launch_stats_chain(hipStream_t s, const ba::ChainParams* cp, const ba::AlignStats* ends, const ba::AlignStats* gaps, ba::AlignStats* out);
// ba_exact.hip, BA_EXACT_UNIT 0 (ba_launch_exact, ba_launch_exact_seed) and 1 (ba_launch_exact_trace, ba_launch_exact_runs)
hipError_t ba_launch_exact(hipStream_t s, const ba::ExactParams* xp, uint32_t wgs);
hipError_t ba_launch_exact_trace(hipStream_t s, const ba::ExactParams* xp, uint32_t waves);
hipError_t ba_launch_exact_runs(hipStream_t s, const uint32_t* rev, const uint64_t* rev_off, const uint32_t* nrun, const uint64_t* off, uint32_t* runs,
                                uint32_t m);
hipError_t ba_launch_exact_seed(hipStream_t s, const ba::ExtendParams* ep, const uint32_t* which, uint32_t m, int32_t* out);
// ba_exact.hip, BA_EXACT_UNIT 2 (ba_launch_exact_modes) and 3 (the other two)
hipError_t ba_launch_exact_modes(hipStream_t s, const ba::ExactModeParams* mp, uint32_t wgs);
hipError_t ba_launch_exact_modes_trace(hipStream_t s, const ba::ExactModeParams* mp, uint32_t* start_cell, uint32_t waves);
hipError_t ba_launch_exact_join(hipStream_t s, const ba::ExactJoinParams* jp);
// ba_text.hip
hipError_t ba_launch_text_len(hipStream_t s, const ba::TextParams* tp);
hipError_t ba_launch_text_write(hipStream_t s, const ba::TextParams* tp);
hipError_t ba_launch_offsets(hipStream_t s, const uint32_t* len, uint64_t* offsets, uint32_t n);   // k_text_offsets on its own
}
