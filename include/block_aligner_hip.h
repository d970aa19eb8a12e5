/*
 * block_aligner_hip.h — C ABI of the MI355X (gfx950) backend for block-aligner.
 *
 * Part 1 is, symbol for symbol, the reference's C API (/root/reference/c/block_aligner.h, generated from
 * /root/reference/src/ffi.rs): a program written against that header links against libblock_aligner_hip.so
 * unchanged (see tests/c_abi/abi_check.c, a gcc-compiled caller in the style of /root/reference/c/example.c). Every alignment is
 * executed by the HIP kernels in block_aligner_amd/csrc; there is no CPU fallback — if no gfx950 device or
 * HIP runtime is usable the call aborts with a message, like the reference's panic=abort.
 *
 * Part 2 adds what the reference's FFI lacks for the hot path named in BASELINE.json: nucleotide / byte
 * matrices (ffi.rs:5 "do not have bindings yet") and a batch launcher that aligns many independent pairs in
 * one kernel launch (one wavefront per pair). A Rust `simd_hip` backend binds exactly these.
 * Behind a traced run, per-alignment statistics (ba_*_stats) and the CIGAR / MD:Z / cs:Z strings of SAM and PAF output (ba_*_text) are
 * computed on the device as well.
 *
 * Error behaviour: Part 1 functions keep the reference contract (no error codes; a violated precondition
 * aborts the process with the reference's assert message). Part 2 functions return 0 on success and a
 * non-zero code otherwise, with ba_last_error() giving the message.
 */
#ifndef BLOCK_ALIGNER_HIP_H
#define BLOCK_ALIGNER_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Part 1 — the reference C API                                                                           */
/* ------------------------------------------------------------------------------------------------------ */

/* cigar.rs:10-31, c/block_aligner.h:17-57: `enum Operation` with a one-byte representation */
enum Operation
#ifdef __cplusplus
    : uint8_t
#endif
{ Sentinel = 0, M = 1, Eq = 2, X = 3, I = 4, D = 5 };
#ifndef __cplusplus
typedef uint8_t Operation;
#endif

typedef struct AAMatrix AAMatrix;       /* scores.rs:40-44: 27 x 32 int8, 32-byte aligned, 864 bytes */
typedef struct NucMatrix NucMatrix;     /* scores.rs:142-146: 8 x 16 int8, 32-byte aligned, 128 bytes */
typedef struct AAProfile AAProfile;     /* opaque */
typedef struct Cigar Cigar;             /* opaque */
typedef struct PaddedBytes PaddedBytes; /* opaque */

typedef struct OpLen { Operation op; uintptr_t len; } OpLen;                                   /* cigar.rs:34-39 */
typedef void* BlockHandle;                                                                      /* ffi.rs:15 */
typedef struct Gaps { int8_t open; int8_t extend; } Gaps;                                       /* scores.rs:333-338 */
typedef struct SizeRange { uintptr_t min; uintptr_t max; } SizeRange;                           /* ffi.rs:18-23 */
typedef struct AlignResult { int32_t score; uintptr_t query_idx; uintptr_t reference_idx; } AlignResult; /* scan_block.rs:1887-1893 */
typedef struct ByteMatrix { int8_t match_score; int8_t mismatch_score; } ByteMatrix;           /* scores.rs:220-225 */

/* data symbols (scores.rs:275-311, c/block_aligner.h:140-162); C callers take their address */
extern const struct NucMatrix NW1;
extern const struct AAMatrix BLOSUM45, BLOSUM50, BLOSUM62, BLOSUM80, BLOSUM90;
extern const struct AAMatrix PAM100, PAM120, PAM160, PAM200, PAM250;
extern const struct ByteMatrix BYTES1;

/* AAMatrix — ffi.rs:31-48 */
struct AAMatrix* block_new_simple_aamatrix(int8_t match_score, int8_t mismatch_score);
void block_set_aamatrix(struct AAMatrix* matrix, uint8_t a, uint8_t b, int8_t score);
void block_free_aamatrix(struct AAMatrix* matrix);

/* AAProfile — ffi.rs:60-195 */
struct AAProfile* block_new_aaprofile(uintptr_t str_len, uintptr_t block_size, int8_t gap_extend);
uintptr_t block_len_aaprofile(const struct AAProfile* profile);
void block_clear_aaprofile(struct AAProfile* profile, uintptr_t str_len, uintptr_t block_size);
void block_set_aaprofile(struct AAProfile* profile, uintptr_t i, uint8_t b, int8_t score);
void block_set_all_aaprofile(struct AAProfile* profile, const uint8_t* order, uintptr_t order_len, const int8_t* scores,
                             uintptr_t scores_len, uintptr_t left_shift, uintptr_t right_shift);
void block_set_all_rev_aaprofile(struct AAProfile* profile, const uint8_t* order, uintptr_t order_len, const int8_t* scores,
                                 uintptr_t scores_len, uintptr_t left_shift, uintptr_t right_shift);
void block_set_gap_open_C_aaprofile(struct AAProfile* profile, uintptr_t i, int8_t gap);
void block_set_gap_close_C_aaprofile(struct AAProfile* profile, uintptr_t i, int8_t gap);
void block_set_gap_open_R_aaprofile(struct AAProfile* profile, uintptr_t i, int8_t gap);
void block_set_all_gap_open_C_aaprofile(struct AAProfile* profile, int8_t gap);
void block_set_all_gap_close_C_aaprofile(struct AAProfile* profile, int8_t gap);
void block_set_all_gap_open_R_aaprofile(struct AAProfile* profile, int8_t gap);
int8_t block_get_aaprofile(const struct AAProfile* profile, uintptr_t i, uint8_t b);
int8_t block_get_gap_extend_aaprofile(const struct AAProfile* profile);
void block_free_aaprofile(struct AAProfile* profile);

/* Cigar — ffi.rs:201-225 */
struct Cigar* block_new_cigar(uintptr_t query_len, uintptr_t reference_len);
struct OpLen block_get_cigar(const struct Cigar* cigar, uintptr_t i);
uintptr_t block_len_cigar(const struct Cigar* cigar);
void block_free_cigar(struct Cigar* cigar);

/* PaddedBytes (amino acids) — ffi.rs:231-257 */
struct PaddedBytes* block_new_padded_aa(uintptr_t len, uintptr_t max_size);
void block_set_bytes_padded_aa(struct PaddedBytes* padded, const uint8_t* s, uintptr_t len, uintptr_t max_size);
void block_set_bytes_rev_padded_aa(struct PaddedBytes* padded, const uint8_t* s, uintptr_t len, uintptr_t max_size);
void block_free_padded_aa(struct PaddedBytes* padded);

/* Block<TRACE, X_DROP> over AAMatrix / AAProfile — ffi.rs:262-403 (gen_functions! x 4) */
#define BA_DECLARE_BLOCK_FNS(S, CIG, CIGEQ)                                                                                   \
    BlockHandle block_new_##S(uintptr_t query_len, uintptr_t reference_len, uintptr_t max_size);                              \
    void block_align_##S(BlockHandle b, const struct PaddedBytes* q, const struct PaddedBytes* r, const struct AAMatrix* m,   \
                         struct Gaps g, struct SizeRange s, int32_t x);                                                       \
    void block_align_profile_##S(BlockHandle b, const struct PaddedBytes* q, const struct AAProfile* r, struct SizeRange s,   \
                                 int32_t x);                                                                                  \
    struct AlignResult block_res_##S(BlockHandle b);                                                                          \
    void CIG(BlockHandle b, uintptr_t query_idx, uintptr_t reference_idx, struct Cigar* cigar);                               \
    void CIGEQ(BlockHandle b, const struct PaddedBytes* q, const struct PaddedBytes* r, uintptr_t query_idx,                  \
               uintptr_t reference_idx, struct Cigar* cigar);                                                                 \
    void block_free_##S(BlockHandle b);

BA_DECLARE_BLOCK_FNS(aa, _block_cigar_aa, _block_cigar_eq_aa)                                   /* ffi.rs:333-349 */
BA_DECLARE_BLOCK_FNS(aa_xdrop, _block_cigar_aa_xdrop, _block_cigar_eq_aa_xdrop)                 /* ffi.rs:351-367 */
BA_DECLARE_BLOCK_FNS(aa_trace, block_cigar_aa_trace, block_cigar_eq_aa_trace)                   /* ffi.rs:369-385 */
BA_DECLARE_BLOCK_FNS(aa_trace_xdrop, block_cigar_aa_trace_xdrop, block_cigar_eq_aa_trace_xdrop) /* ffi.rs:387-403 */

/* ------------------------------------------------------------------------------------------------------ */
/* Part 2 — extensions for the MI355X hot path                                                            */
/* ------------------------------------------------------------------------------------------------------ */

/* thread-local message for the last failing Part 2 call */
const char* ba_last_error(void);
/* 1 for the development build of the library (lib/libblock_aligner_hip_dev.so: reads the BA_* switches, tests and tools only), 0 for the
 * release library, which reads no environment variables. */
int ba_dev_build(void);
/* Hash of the kernel sources this library was built from (tools/kernel_hash.py at build time): equal for the release and the
 * development library of one build. */
const char* ba_build_id(void);
/* Page-locked host memory for result buffers (device-to-host copies into it run at PCIe speed; into pageable memory at a fraction). */
void* ba_host_alloc(uint64_t bytes);
void ba_host_free(void* p);
/* number of usable HIP devices (0 if the runtime is unusable); ba_set_device selects the one later calls OF THE CALLING
 * THREAD use (the selection is per host thread, so one thread can drive each GPU) */
int ba_device_count(void);
int ba_set_device(int device);
/* free / total bytes of the selected device's memory (hipMemGetInfo) */
int ba_device_memory(uint64_t* free_bytes, uint64_t* total_bytes);
/* lib.rs:109-111 */
uintptr_t block_percent_len(uintptr_t len, float p);

/* Nucleotide / byte matrices and padded strings (the reference has Rust API only: scores.rs:142-273,
 * scan_block.rs:1798-1822 instantiated with NucMatrix / ByteMatrix). */
struct NucMatrix* block_new_simple_nucmatrix(int8_t match_score, int8_t mismatch_score);
void block_set_nucmatrix(struct NucMatrix* matrix, uint8_t a, uint8_t b, int8_t score);
void block_free_nucmatrix(struct NucMatrix* matrix);
struct PaddedBytes* block_new_padded_nuc(uintptr_t len, uintptr_t max_size);
void block_set_bytes_padded_nuc(struct PaddedBytes* padded, const uint8_t* s, uintptr_t len, uintptr_t max_size);
void block_set_bytes_rev_padded_nuc(struct PaddedBytes* padded, const uint8_t* s, uintptr_t len, uintptr_t max_size);
void block_free_padded_nuc(struct PaddedBytes* padded);
struct PaddedBytes* block_new_padded_bytes(uintptr_t len, uintptr_t max_size);
void block_set_bytes_padded_bytes(struct PaddedBytes* padded, const uint8_t* s, uintptr_t len, uintptr_t max_size);
void block_free_padded_bytes(struct PaddedBytes* padded);

/* mode bits of Block<TRACE, X_DROP, LOCAL_START, FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS> (scan_block.rs:89) */
enum {
    BA_TRACE = 1u << 0,
    BA_X_DROP = 1u << 1,
    BA_LOCAL_START = 1u << 2,
    BA_FREE_QUERY_START_GAPS = 1u << 3,
    BA_FREE_QUERY_END_GAPS = 1u << 4,
    BA_CIGAR_EQ = 1u << 5 /* batch only: emit =/X instead of M (Trace::cigar_eq, scan_block.rs:1478-1480) */
};
enum { BA_KIND_AA = 0, BA_KIND_NUC = 1, BA_KIND_BYTES = 2 };

/* Generic per-pair block: Block::<mode>::new / align::<matrix kind> / res / trace().cigar[_eq]
 * (scan_block.rs:798-805, 847-878, 1235-1244, 1469-1480). `matrix` points at an AAMatrix, NucMatrix or
 * ByteMatrix according to `kind`; q and r must have been built for the same kind. */
BlockHandle block_new_generic(uint32_t mode, uintptr_t query_len, uintptr_t reference_len, uintptr_t max_size);
void block_align_generic(BlockHandle b, int kind, const struct PaddedBytes* q, const struct PaddedBytes* r, const void* matrix,
                         struct Gaps g, struct SizeRange s, int32_t x);
struct AlignResult block_res_generic(BlockHandle b);
/* Block::<mode>::align_profile (scan_block.rs:942-968): q must be an AA PaddedBytes; the gap costs come from the profile. */
void block_align_profile_generic(BlockHandle b, const struct PaddedBytes* q, const struct AAProfile* profile, struct SizeRange s,
                                 int32_t x);
/* The same two calls for a caller that keeps its own PaddedBytes (the Rust crate behind the `simd_hip` feature, rust/src/): the padded
 * image as the reference stores it -- [NULL] + converted bytes + NULL x block_size (src/scan_block.rs:1790-1812) -- passed by pointer
 * (q_s[0] is the NULL pad; q_len the sequence length). */
void block_align_padded_generic(BlockHandle b, int kind, const uint8_t* q_s, uintptr_t q_len, const uint8_t* r_s, uintptr_t r_len,
                                const void* matrix, struct Gaps g, struct SizeRange s, int32_t x);
void block_align_profile_padded_generic(BlockHandle b, const uint8_t* q_s, uintptr_t q_len, const struct AAProfile* profile,
                                        struct SizeRange s, int32_t x);
void block_cigar_generic(BlockHandle b, uintptr_t query_idx, uintptr_t reference_idx, struct Cigar* cigar);
void block_cigar_eq_generic(BlockHandle b, const struct PaddedBytes* q, const struct PaddedBytes* r, uintptr_t query_idx,
                            uintptr_t reference_idx, struct Cigar* cigar);
void block_free_generic(BlockHandle b);
/* Trace::blocks() (scan_block.rs:1676-1691): the rectangles computed for the last alignment, in fill order. Returns their
 * number; writes at most `capacity` of them (out may be NULL to query the count). */
struct Rectangle { uintptr_t row, col, width, height; };
uintptr_t block_trace_blocks_generic(BlockHandle b, struct Rectangle* out, uintptr_t capacity);

/* ---- batch launcher: many independent pairs, one persistent kernel launch, one wavefront per pair.
 *
 * `pool` holds the raw (unpadded, unconverted) sequence bytes; pair p is query pool[q_off[p] .. +q_len[p]) against
 * reference pool[r_off[p] .. +r_len[p]). The library builds the PaddedBytes images (scan_block.rs:1798-1812: convert_char,
 * NULL pads; on the device when the pairs come out of one dense buffer, a byte outside the alphabet is an error) and keeps
 * them, the matrix and all scratch resident in device memory for the life of the batch object, so ba_batch_run can
 * be timed with inputs already in HBM.
 *
 * Results per pair: score / query_idx / reference_idx as AlignResult (scan_block.rs:567-592); computed DP cells
 * (sum over every block-fill call of columns iterated x height: the GCUPS numerator); CIGAR runs when BA_TRACE is set,
 * each run packed as (len << 4 | Operation), in alignment order. */
typedef struct BaBatch BaBatch;

BaBatch* ba_batch_create(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, uint32_t mode,
                         const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                         const uint32_t* r_len, uintptr_t n_pairs);
/* Bulk form of block_set_aaprofile / block_set_gap_*_aaprofile for callers that hold the profile as arrays: copies the
 * first `positions` rows of pos_aa ([position][32], column = byte - 'A') and entries of the three gap arrays. */
int ba_aaprofile_set_raw(struct AAProfile* profile, const int8_t* pos_aa, const int8_t* gap_open_C, const int8_t* gap_close_C,
                         const int8_t* gap_open_R, uintptr_t positions);

/* Sequence-to-profile batch (Block::align_profile over many pairs; examples/pssm_bench.rs:86-103): pair p aligns the
 * amino-acid query pool[q_off[p] .. +q_len[p]) to *profiles[p]. Every profile must have been created with a block size
 * >= size.max and share one gap_extend. The profiles are copied to the device; the caller keeps ownership.
 * BA_CIGAR_EQ is rejected (there is no second sequence to compare with). */
BaBatch* ba_batch_create_profile(const struct AAProfile* const* profiles, struct SizeRange size, int32_t x_drop, uint32_t mode,
                                 const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n_pairs);
/* Replace the pairs of an existing batch and keep its device buffers (the trace arena above all, whose allocation
 * dominates the set-up time): same matrix, gaps, block range and modes. The new set must fit what the batch was created
 * with: no more pairs, no more sequence bytes in total, no pair longer than the longest original one. */
int ba_batch_reload(BaBatch* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                    const uint32_t* r_len, uintptr_t n_pairs);
int ba_batch_reload_profile(BaBatch* batch, const struct AAProfile* const* profiles, const uint8_t* pool, const uint64_t* q_off,
                            const uint32_t* q_len, uintptr_t n_pairs);
/* Launch on the batch's stream and wait. kernel_ms (optional) = HIP-event time of the alignment kernel alone. */
int ba_batch_run(BaBatch* batch, float* kernel_ms);
/* The two halves of ba_batch_run: enqueue on the batch's own stream and return / wait for it. Launches of different
 * batches overlap on the device; results, cigars and reload are valid after the wait.
 * Which calls are valid when:
 *   no results (created, reloaded, or the last wait failed): ba_batch_launch, ba_batch_run, ba_batch_reload, ba_batch_exact*; every getter of a
 *     run's results is refused.
 *   in flight (ba_batch_launch returned 0, no ba_batch_wait has succeeded or ended in an error since -- a wait that timed out leaves the batch
 *     here): ba_batch_wait and ba_batch_compact_cigars. ba_batch_results, _cigars, _surviving_cells, _spec_cells, _skipped_cells, _prof, _stats,
 *     _text, _exact*, _reload, _launch and _run are refused with "launch in flight (ba_batch_wait first)" before they touch the device: the
 *     kernels are still writing what they would read, and the batch's stream is non-blocking.
 *   results (a ba_batch_wait or ba_batch_run returned 0): everything but ba_batch_wait and ba_batch_compact_cigars.
 *   ba_batch_info, _kernel, _geometry and _retried (the count of the last COMPLETED run) read host state and answer in every state.
 * ba_batch_launch takes the results of the run before away: from then on the batch has none until a wait succeeds, whatever becomes of the launch.
 * At most TWO launches in flight per device if they are BA_TRACE batches of more than a few pairs per resident wave: such a launch's waves wait for each other
 * (the traceback waves for the fill waves' hand-offs, k_multi's idle waves for its last fill wave), so it must become fully resident to end. The first launch
 * on an idle device is; a second one follows it; three or more may each hold a part of the device and keep each other's remaining workgroups out
 * (ba_sized_batch_run orders its ranges' launches accordingly). Score-only batches have no such waits. */
int ba_batch_launch(BaBatch* batch);
int ba_batch_wait(BaBatch* batch, float* kernel_ms);
/* Upper bound on a ba_batch_wait / ba_batch_run (milliseconds; default 600000; 0 = none): the kernels of a launch wait for each other without a
 * give-up, so the host bounds the wait -- past it the call fails (ba_last_error) instead of never returning. Process-wide. A timeout is not a failed
 * launch: the batch stays in flight (results and a relaunch are refused; a later ba_batch_wait may still succeed -- raise the limit, or pass 0, for
 * launches that legitimately take longer), and ba_batch_destroy blocks until the device has let go of the batch's memory. */
void ba_set_wait_limit_ms(uint64_t ms);
/* Copy results to host arrays of n_pairs elements; any pointer may be NULL. status: 0 = ok, else BA_ST_* bits. */
int ba_batch_results(BaBatch* batch, int32_t* score, uint32_t* query_idx, uint32_t* reference_idx, uint64_t* cells,
                     uint32_t* cigar_len, uint32_t* status);
/* CIGAR runs of all pairs, concatenated in pair order (pair p occupies cigar_len[p] entries after the pairs before it).
 * `capacity` = number of uint32 entries available in `runs`; fails if too small. */
int ba_batch_cigars(BaBatch* batch, uint32_t* runs, uint64_t capacity);
/* Optional, between ba_batch_launch and ba_batch_wait: gather the CIGAR runs on the device right behind the alignment kernels -- into
 * `pinned_out` (memory from ba_host_alloc, capacity in runs; after ba_batch_wait the runs are in host memory and ba_batch_cigars on the same
 * pointer copies nothing), or with pinned_out = NULL into a device buffer (ba_batch_cigars is then one device-to-host copy). Either way no
 * kernel or copy has to find room beside another batch's launch afterwards. */
int ba_batch_compact_cigars(BaBatch* batch, uint32_t* pinned_out, uint64_t pinned_capacity);
/* TRACE batches: per pair, the sum of width x height over the rectangles left on its trace stack (Trace::blocks(),
 * scan_block.rs:1676-1691; the numerator of the reference's "DP fraction", examples/uc_accuracy.rs:88-89). */
int ba_batch_surviving_cells(BaBatch* batch, uint64_t* cells);
/* Facts about the launch: out[0] grid (resident waves), [1] LDS bytes per wave, [2] trace arena bytes, [3] padded pool bytes */
int ba_batch_info(BaBatch* batch, uint64_t out[4]);
/* Which fill kernel the batch's launches use: 0 the per-pair kernel (k_align), 1 four pairs per wave at 128 cells (k_multi), 2 the round-2/3
 * small-block pipeline (k_quad + queue; profile batches), 3 sixteen pairs per wave at 32 cells (k_small). -1 for a null batch. */
int ba_batch_kernel(BaBatch* batch);
/* k_multi batches: the launch geometry chosen for the batch size -- 0: eight-wave workgroups at four waves per SIMD (batches of many rounds); 3 / 2: four-wave
 * workgroups at three / two waves per SIMD (DNA, block classes 512 and 1024: batches whose pairs fill that many waves' slots about once). -1 for a null batch. */
int ba_batch_geometry(BaBatch* batch);
/* X-drop + BA_TRACE batches: cells of the last run's speculative, untraced rectangles (the chain of grows that closes an X-drop alignment
 * can lie on no path: filled without trace flags and location bookkeeping) -- a part of the computed cells that needed 14 instead of 20
 * int16 operations per cell (bench.py: roofline.ops_required). */
int ba_batch_spec_cells(BaBatch* batch, uint64_t* cells);
/* X-drop batches over a NucMatrix or an AAMatrix whose padding byte scores below 0 against every byte (new_simple and the stock matrices do):
 * cells of the last run that were NOT computed -- the columns past the sequence ends in the block that closes an alignment, which can hold
 * no new best. They are counted in the pairs' `cells` all the same (the reference computes them). 0 for every other batch. */
int ba_batch_skipped_cells(BaBatch* batch, uint64_t* cells);
/* Large TRACE batches size their trace slots for the expected stack, not for the reference's worst case (Trace::new,
 * scan_block.rs:1363-1366); pairs that outgrow a slot are re-run with full-size slots inside ba_batch_run / ba_batch_wait. (Large: from 4096 pairs, or
 * from 256 pairs of 10 kbp and more.) Likewise a batch whose block range starts at 128 .. 1024 cells and ends above 2048 is launched in the 2048-cell class;
 * pairs whose block wants to grow past 2048 cells are re-run in the row-tiled class, and a batch of which more than an eighth did is launched in the
 * row-tiled class from its next run on.
 * Number of pairs the last run re-ran (results are identical either way; -1 for a null batch). */
int ba_batch_retried(BaBatch* batch);
void ba_batch_destroy(BaBatch* batch);

/* ---- seed-and-extend batches: X-drop extension on both sides of a seed, one result per seed ("Seed extension").
 *
 * Seed p lies at q[q_seed[p] .. + seed_len[p]) of its query q = pool[q_off[p] .. +q_len[p]) and r[r_seed[p] .. + seed_len[p]) of its reference
 * r = pool[r_off[p] .. +r_len[p]); seed_len >= 1, and the seed lies inside both sequences. strand (NULL = all 0; NucMatrix batches only):
 * strand[p] = 1 replaces q by its reverse complement (uppercased bytes, A <-> T, C <-> G, every other letter as it is) before anything else;
 * seed coordinates and results are in that oriented frame. The seed is an ungapped anchor (it need not be an exact match): its score is the
 * sum of matrix(q[q_seed + k], r[r_seed + k]). Left side: Block::<TRACE, true>::align of rev(q[0 .. q_seed)) against rev(r[0 .. r_seed)); right
 * side: the same alignment of q[q_seed + seed_len ..] against r[r_seed + seed_len ..]; a side where either sequence is empty is not aligned
 * (score 0, end (0, 0), no cells, no runs). All non-empty sides of a set are ONE ordinary batch on the device -- the images are cut out of the
 * caller's bytes there, and the seeds and both sides are spliced there.
 *
 * Modes: BA_X_DROP is required, BA_TRACE and BA_CIGAR_EQ are optional; LOCAL_START and FREE_QUERY_* are rejected, and so are profile batches.
 * Every argument is checked before the device is touched (a seed out of range, seed_len 0, strand on another matrix: a message naming the seed). */
typedef struct BaExtendBatch BaExtendBatch;
BaExtendBatch* ba_extend_batch_create(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, uint32_t mode,
                                      const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                      const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, const uint8_t* strand, uintptr_t n_seeds);
/* Replace the seeds and keep the device buffers, as ba_batch_reload: the new set must fit what the batch was created with -- no more seeds,
 * no more sequence bytes, and its sides no more than the original sides (in number, bytes and longest pair). */
int ba_extend_batch_reload(BaExtendBatch* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                           const uint32_t* r_len, const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, const uint8_t* strand,
                           uintptr_t n_seeds);
/* Fill both sides of every seed (one launch, re-runs included), then splice. kernel_ms (optional) = HIP-event time of the fill, as ba_batch_run. */
int ba_extend_batch_run(BaExtendBatch* batch, float* kernel_ms);
/* Results per seed, in the caller's order; any pointer may be NULL. score = left_score + seed score + right_score; the alignment covers
 * q[q_start .. q_end) and r[r_start .. r_end) (q_start = q_seed - the left side's query end, q_end = q_seed + seed_len + the right side's
 * query end; likewise r); cells = both sides' cells; status = the OR of both sides' BA_ST_* bits; cigar_len = runs per seed (BA_TRACE). */
int ba_extend_batch_results(BaExtendBatch* batch, int32_t* score, uint32_t* q_start, uint32_t* r_start, uint32_t* q_end, uint32_t* r_end,
                            int32_t* left_score, int32_t* right_score, uint64_t* cells, uint32_t* cigar_len, uint32_t* status);
/* BA_TRACE: every seed's runs, concatenated in seed order (as ba_batch_cigars): the left side's runs reversed, the seed as one M run (its =/X
 * runs with BA_CIGAR_EQ), the right side's runs; adjacent runs with the same op merged at both joins. Rescored over q[q_start .. q_end) /
 * r[r_start .. r_end), the runs give `score` exactly. */
int ba_extend_batch_cigars(BaExtendBatch* batch, uint32_t* runs, uint64_t capacity);
/* Device times in ms: the last run's fill (as kernel_ms) and splice; the image packers of the last create / reload. Any pointer may be NULL. */
int ba_extend_batch_times(BaExtendBatch* batch, float* fill_ms, float* pack_ms, float* splice_ms);
void ba_extend_batch_destroy(BaExtendBatch* batch);

/* ---- anchor-chain batches: global alignment between the anchors of a chain, X-drop extension at its two ends, one result per chain
 * ("Anchor chains").
 *
 * Chain c holds the K >= 1 anchors anchor_first[c] .. anchor_first[c + 1] (anchor_first: n_chains + 1 entries, from 0, increasing). Anchor k
 * lies at q[q_anchor .. + anchor_len) and r[r_anchor .. + anchor_len) of the chain's query q = pool[q_off[c] .. +q_len[c]) and reference
 * r = pool[r_off[c] .. +r_len[c]), anchor_len >= 1; the anchors of a chain are colinear and disjoint on both sequences (anchor k ends at or
 * before the start of anchor k + 1) and lie inside them. strand as for ba_extend_batch_create: strand[c] = 1 (NucMatrix only) replaces q by its
 * reverse complement, and the anchors and the results are in that frame.
 *
 * An anchor is ungapped and need not match exactly: its score is the sum of matrix(q, r) over its columns. Gap k, between anchors k and k + 1,
 * has the slices gq = q[end of k .. start of k + 1) and gr likewise: both empty -- nothing; one empty -- one I run (gr empty) or one D run (gq
 * empty) over the other's length d, score open + (d - 1) * extend, no cells; both non-empty -- Block::<TRACE, false>::align of gq against gr with
 * the batch's matrix, gaps and block range, without X-drop, ending at its corner. The ends are the two sides of a seed (above): left of anchor 0
 * the reversed prefixes, right of anchor K - 1 the suffixes, each with X-drop; an empty side is not aligned. All ends of a set are ONE X-drop
 * batch on the device and all aligned gaps ONE global batch, their images cut out of the caller's bytes there; the fills run one after the
 * other, and everything is spliced on the device. A chain of one anchor is a seed: results and runs are ba_extend_batch_*'s, bit for bit.
 *
 * Modes: BA_X_DROP is required (for the ends), BA_TRACE and BA_CIGAR_EQ are optional; LOCAL_START and FREE_QUERY_* are rejected, and so are
 * profile batches. The gap batch has the same mode without BA_X_DROP. Every argument is checked before the device is touched (a chain without
 * anchors, anchor_len 0, anchors that overlap or are out of order, an anchor past the end, anchor_first that does not start at 0 or decreases,
 * a bad strand: a message naming the chain and the anchor). */
typedef struct BaChainBatch BaChainBatch;
BaChainBatch* ba_chain_batch_create(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, uint32_t mode,
                                    const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                    const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len,
                                    const uint8_t* strand, uintptr_t n_chains);
/* Replace the chains and keep the device buffers, as ba_extend_batch_reload: the new set must fit what the batch was created with -- no more
 * chains, anchors or sequence bytes, and its ends and its aligned gaps no more than the original ones (in number, bytes and longest pair); a
 * batch created without ends (or without aligned gaps) takes no set that has some. */
int ba_chain_batch_reload(BaChainBatch* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                          const uint32_t* r_len, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                          const uint32_t* anchor_len, const uint8_t* strand, uintptr_t n_chains);
/* Fill the ends, then the gaps (re-runs included), then splice. kernel_ms (optional) = HIP-event time of both fills. */
int ba_chain_batch_run(BaChainBatch* batch, float* kernel_ms);
/* Results per chain, in the caller's order; any pointer may be NULL. score = both ends + all anchors + all gaps; the alignment covers
 * q[q_start .. q_end) and r[r_start .. r_end), taken from the first and the last anchor as for a seed; left_score / right_score = the ends'
 * scores; cells = the sum over all aligned pieces; status = the OR of their BA_ST_* bits; cigar_len = runs per chain (BA_TRACE). */
int ba_chain_batch_results(BaChainBatch* batch, int32_t* score, uint32_t* q_start, uint32_t* r_start, uint32_t* q_end, uint32_t* r_end,
                           int32_t* left_score, int32_t* right_score, uint64_t* cells, uint32_t* cigar_len, uint32_t* status);
/* BA_TRACE: every chain's runs, concatenated in chain order: the left end's runs reversed, anchor 0, gap 0, anchor 1, ..., anchor K - 1, the
 * right end's runs (an anchor: one M run, or its =/X runs with BA_CIGAR_EQ); adjacent runs with the same op are merged at every join, across
 * any number of pieces. Every gap lies between two anchors, so two gap runs never merge and every merge is score-neutral: rescored over
 * q[q_start .. q_end) / r[r_start .. r_end), the runs give `score` exactly. */
int ba_chain_batch_cigars(BaChainBatch* batch, uint32_t* runs, uint64_t capacity);
/* Device times in ms: the last run's two fills and its splice; the image packers of the last create / reload. Any pointer may be NULL. */
int ba_chain_batch_times(BaChainBatch* batch, float* ends_ms, float* gaps_ms, float* pack_ms, float* splice_ms);
/* (The statistics and the CIGAR / MD / cs strings of the chains: ba_chain_batch_stats, ba_chain_batch_text and ba_chain_batch_report_ms,
 * declared with the other ba_*_stats and ba_*_text calls below.) */
void ba_chain_batch_destroy(BaChainBatch* batch);

/* ---- colinear anchor chaining on the device: from the raw hits of a problem (one read against one reference on one strand: a future row of a
 * chain batch) to its best colinear chains, in the array layout ba_chain_batch_create takes ("Chaining anchors": the rule).
 *
 * Problem p holds the anchors anchor_first[p] .. anchor_first[p + 1] (n_problems + 1 entries, from 0, never decreasing; a problem may be
 * empty), anchor_len >= 1. With qe = q_anchor + anchor_len and re = r_anchor + anchor_len, the anchors of a problem are sorted by (re, qe)
 * ascending (equal keys allowed), qe and re stay below 2^31, match_w * the sum of a problem's anchor_len stays below 2^31 and
 * drift_cost * bandwidth + skip_cost * max_dist below 2^30. Every argument is checked before the device is touched; a message names the
 * problem and the anchor. Scores are exact int32 arithmetic. */
struct BaChainingParams {
    int32_t match_w;       /* >= 1: what a column of an anchor is worth */
    int32_t drift_cost;    /* >= 0: per diagonal between consecutive anchors, |dq - dr| */
    int32_t skip_cost;     /* >= 0: per column skipped between consecutive anchors, min(dq, dr) - gain */
    uint32_t lookback;     /* 1 .. 1024: the anchors before an anchor that may precede it (H) */
    uint32_t max_dist;     /* >= 1: dq, dr <= max_dist */
    uint32_t bandwidth;    /* |dq - dr| <= bandwidth */
    uint32_t max_chains;   /* 1 .. 64: candidates walked per problem */
    int32_t min_score;     /* a chain is kept from this score */
    uint32_t min_anchors;  /* >= 1: ... and from this many anchors */
};
typedef struct BaChaining BaChaining;
BaChaining* ba_chaining_create(const struct BaChainingParams* params, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                               const uint32_t* anchor_len, uintptr_t n_problems);
/* Replace the problems and keep parameters and device buffers: the new set must hold no more problems and no more anchors. */
int ba_chaining_reload(BaChaining* batch, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len,
                       uintptr_t n_problems);
/* The fill, the pick, the offsets and the gather. kernel_ms (optional): the sum of their HIP-event times. */
int ba_chaining_run(BaChaining* batch, float* kernel_ms);
/* After a run: kept chains, their anchors, and the chains of every problem (n_problems entries). Any pointer may be NULL. */
int ba_chaining_counts(BaChaining* batch, uint64_t* n_chains, uint64_t* n_anchors, uint32_t* chains_per_problem);
/* After a run; any pointer may be NULL. Per kept chain (n_chains entries; problems in order, the chains of a problem in the order picked):
 * its problem, its rank within the problem and its score; out_anchor_first (n_chains + 1 entries): where its anchors start. Per kept anchor
 * (n_anchors entries, in path order): the anchor trimmed to its gain -- disjoint from and colinear with the one before it on both
 * sequences, at least one column -- and out_anchor_src, the input anchor it came from (an index within its problem).
 * chain_problem expands per-problem arrays to per-chain ones; out_anchor_first, out_q_anchor, out_r_anchor and out_anchor_len are
 * ba_chain_batch_create's arguments as they stand. */
int ba_chaining_results(BaChaining* batch, uint32_t* chain_problem, uint32_t* chain_rank, int32_t* chain_score, uint64_t* out_anchor_first,
                        uint32_t* out_q_anchor, uint32_t* out_r_anchor, uint32_t* out_anchor_len, uint32_t* out_anchor_src);
/* After a run: the raw fill per input anchor, f and pred (an index within the problem, -1: none). Either pointer may be NULL. */
int ba_chaining_dp(BaChaining* batch, int32_t* f, int32_t* pred);
/* Device times of the last run in ms: the fill, the pick with both offset scans, the gather. Any pointer may be NULL. */
int ba_chaining_times(BaChaining* batch, float* fill_ms, float* pick_ms, float* gather_ms);
void ba_chaining_destroy(BaChaining* batch);

/* ---- minimizer seeding on the device: from the bytes of a problem (one read against one reference stretch on one strand, in the pair layout
 * of ba_chain_batch_create: q = pool[q_off[p] .. + q_len[p]), r likewise, strand[p] or NULL) to its raw hits, in the order ba_chaining_create
 * demands ("Seeding": the rule, normative; all integer arithmetic).
 *
 * With strand[p] = 1 the query is read as its reverse complement (uppercased, A<->T, C<->G, every other byte as it is), and every query
 * position is in that frame: the chain batch's. A k-mer's code takes A, C, G, T (either case) as 0 .. 3, the first base most significant; a
 * k-mer over any other byte is invalid: never selected, never compared. h(x), in uint32: x ^= 0x9e3779b9; x ^= x >> 16; x *= 0x85ebca6b;
 * x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16 (a bijection). A sequence with nk k-mers has the windows [s, s + w) for s = 0 .. nk - w, or the
 * one window [0, nk) if nk <= w; a window selects its valid k-mer with the smallest h, the leftmost of equals; the sketch is the set of
 * selected positions, ascending. Per problem the reference's sketch is walked in position order: an entry (j, c) whose code occurs m times
 * among the query's selected entries gives, if 1 <= m <= max_occ, the hits (q_hit = i, r_hit = j, hit_len = k) for those m positions i,
 * ascending. The hits of a problem are therefore sorted by (r_hit, q_hit), lie inside their sequences and end below 2^31.
 *
 * Every argument is checked before the device is touched (k, w, max_occ out of range; a strand that is not 0 or 1; a sequence of 2^31 - 16
 * bytes or more: a message naming the problem). A set may hold at most 2^28 hits, the chainer's limit: ba_seeding_run fails otherwise. */
struct BaSeedingParams {
    uint32_t k;        /* 4 .. 16: bases of a k-mer */
    uint32_t w;        /* 1 .. 64: k-mers of a window (1: every valid k-mer is selected) */
    uint32_t max_occ;  /* >= 1: a code that more of the query's selected k-mers have gives no hits; 0xffffffff: no cap in practice */
};
typedef struct BaSeeding BaSeeding;
BaSeeding* ba_seeding_create(const struct BaSeedingParams* params, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len,
                             const uint64_t* r_off, const uint32_t* r_len, const uint8_t* strand, uintptr_t n_problems);
/* Replace the problems and keep parameters and device buffers: the new set must hold no more problems and no more sequence bytes. */
int ba_seeding_reload(BaSeeding* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                      const uint32_t* r_len, const uint8_t* strand, uintptr_t n_problems);
/* The sketch of every sequence, the sort of the queries' entries by code, the match. kernel_ms (optional): the sum of their HIP-event times.
 * Fails, naming a problem, if the set has more than 2^28 hits; the batch can be reloaded and run again. */
int ba_seeding_run(BaSeeding* batch, float* kernel_ms);
/* After a run: hits, selected k-mers of all queries and of all references, and the hits of every problem (n_problems entries). Any pointer
 * may be NULL. */
int ba_seeding_counts(BaSeeding* batch, uint64_t* n_hits, uint64_t* n_q_seeds, uint64_t* n_r_seeds, uint32_t* hits_per_problem);
/* After a run; any pointer may be NULL. hit_first (n_problems + 1 entries): where a problem's hits start; per hit (n_hits entries) q_hit, r_hit
 * and hit_len (= k): ba_chaining_create's anchor_first, q_anchor, r_anchor and anchor_len as they stand. */
int ba_seeding_results(BaSeeding* batch, uint64_t* hit_first, uint32_t* q_hit, uint32_t* r_hit, uint32_t* hit_len);
/* After a run: the raw sketches, in position order; any pointer may be NULL. q_seed_first / r_seed_first (n_problems + 1 entries each):
 * where the entries of a problem's query / reference start; per entry (n_q_seeds / n_r_seeds of them) its position and its code. */
int ba_seeding_sketch(BaSeeding* batch, uint64_t* q_seed_first, uint32_t* q_seed_pos, uint32_t* q_seed_code, uint64_t* r_seed_first,
                      uint32_t* r_seed_pos, uint32_t* r_seed_code);
/* Device times of the last run in ms: the sketch's two passes, the sort, the match's two passes (each with its scan). Any pointer may be NULL. */
int ba_seeding_times(BaSeeding* batch, float* sketch_ms, float* sort_ms, float* match_ms);
void ba_seeding_destroy(BaSeeding* batch);
/* The hand-off: a chaining batch over the hits of a seeder that has run, copied device to device on the seeder's device (hit_first is the
 * only thing that passes through the host). match_w * k * the hits of a problem must stay below 2^31. The handle is a BaChaining like any
 * other -- run, counts, results, dp, times, destroy; reload takes host arrays that fit its capacity -- and does not depend on the seeder
 * afterwards: the copy is complete when the call returns, and the seeder may be reloaded, run again or destroyed at once. */
BaChaining* ba_chaining_create_seeded(const struct BaChainingParams* params, BaSeeding* ran);

/* ---- a reference index: the sketch of one reference, built once, and many reads seeded against all of it ("Reference
 * index"). The index holds the (w, k)-minimizer sketch of ref[0 .. ref_len) on strand 0 under the rule of "Seeding", as keys
 * code << 32 | pos in ascending order with a prefix table over the top min(2k, 20) bits of the code; the bytes are not kept. k is 4 .. 16, w
 * is 1 .. 64, ref is not NULL and ref_len is below 2^31 - 16: checked before the device is touched. A reference shorter than k has no entries.
 * Several reference sequences: ba_ref_index_create_multi, below. */
typedef struct BaRefIndex BaRefIndex;
BaRefIndex* ba_ref_index_create(uint32_t k, uint32_t w, const uint8_t* ref, uint64_t ref_len);
/* Any pointer may be NULL. longest_run: the largest number of entries that share one code (what max_ref_occ is compared with). */
int ba_ref_index_counts(BaRefIndex* index, uint64_t* n_entries, uint32_t* k, uint32_t* w, uint64_t* ref_len, uint32_t* longest_run);
/* The entries, n_entries each, ascending by (code, pos). Either pointer may be NULL. */
int ba_ref_index_entries(BaRefIndex* index, uint32_t* code, uint32_t* pos);
/* Device times of the build in ms: the sketch's two passes, the sort of the keys, the prefix table. Any pointer may be NULL. */
int ba_ref_index_times(BaRefIndex* index, float* sketch_ms, float* sort_ms, float* table_ms);
/* Seeders made from the index share its device buffers and stay valid. */
void ba_ref_index_destroy(BaRefIndex* index);
/* A seeder whose problem p is read p = pool[q_off[p] .. + q_len[p]) on strand[p] (or NULL) against the whole indexed reference; k and w are
 * the index's. The hits are those of ba_seeding_create with r the whole reference, except that a reference entry whose code occurs more
 * than max_ref_occ times in the reference's sketch gives none (max_ref_occ >= 1; 0xffffffff: no cap, and then the hits are equal bit for
 * bit). The handle is a BaSeeding on the index's device: run, counts, results, sketch (no reference entries: n_r_seeds is 0 and r_seed_first
 * all zeros), times (the sketch; the sorts of the queries' keys and of the hits; the lookup), destroy and ba_chaining_create_seeded work on
 * it. ba_seeding_reload refuses it and ba_seeding_reload_indexed refuses any other seeder. The other arguments are checked before the index
 * is looked at. */
BaSeeding* ba_seeding_create_indexed(BaRefIndex* index, uint32_t max_occ, uint32_t max_ref_occ, const uint8_t* pool, const uint64_t* q_off,
                                     const uint32_t* q_len, const uint8_t* strand, uintptr_t n_problems);
int ba_seeding_reload_indexed(BaSeeding* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint8_t* strand,
                              uintptr_t n_problems);
/* Candidate windows (host only): the stretch of its reference that a chain can reach, so that ba_chain_batch_create packs no more than that.
 * Chain c has the first anchor (qa0, ra0) and its last anchor ends at (qe, re); in 64-bit arithmetic lo = ra0 - min(ra0, qa0 + margin),
 * hi = re + min(r_len - re, (q_len - qe) + margin), r_off_out = r_off + lo, r_len_out = hi - lo, r_anchor_out = r_anchor - lo. A chain without
 * anchors or an anchor that ends outside its sequences is refused with the chain's number. The outputs, with the other arguments as they
 * are, are a valid input of ba_chain_batch_create; reference positions of its results are relative to r_off_out. */
int ba_chain_windows(const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, const uint64_t* anchor_first, const uint32_t* q_anchor,
                     const uint32_t* r_anchor, const uint32_t* anchor_len, uintptr_t n_chains, uint32_t margin, uint64_t* r_off_out,
                     uint32_t* r_len_out, uint32_t* r_anchor_out);

/* ---- several reference sequences in one index ("Several sequences": the rule, normative). The sequences
 * seq[s] = pool[seq_off[s] .. + seq_len[s]) are laid end to end without a spacer: seq_start[0] = 0, seq_start[s + 1] = seq_start[s] +
 * seq_len[s]. Every reference position downstream -- index entries, r_hit, chain anchors -- is in that frame until it is located. The
 * entries are the union of the entries of every sequence alone, shifted by its start: no k-mer and no window holds bytes of two sequences;
 * longest_run, the prefix table and max_ref_occ count over all of them together. n_seqs is 1 .. 2^20, empty sequences are legal, and
 * seq_start[n_seqs] stays below 2^31 - 16; every argument is checked before the device is touched. One sequence gives the index of
 * ba_ref_index_create bit for bit. The pool need not hold the sequences contiguously or in order. A seeder made from such an index
 * (ba_seeding_create_indexed, unchanged) carries the sequence table, and ba_chaining_create_seeded on it makes a bounded chainer. */
BaRefIndex* ba_ref_index_create_multi(uint32_t k, uint32_t w, const uint8_t* pool, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs);
/* Any index's sequences: their number and where they start in the index's frame (n_seqs + 1 entries, the last one the end; or NULL). An
 * index made by ba_ref_index_create has one, from 0 to ref_len. */
int ba_ref_index_sequences(BaRefIndex* index, uint64_t* n_seqs, uint64_t* seq_start);
/* ba_chaining_create for anchors in the frame of a sequence table (n_seqs + 1 ascending entries from 0, n_seqs 1 .. 2^20, the last below
 * 2^31 - 16): the fill admits a predecessor j of anchor i only if it ends behind the start of the sequence that holds i -- the last
 * non-empty sequence that starts at or before i's reference position --, so every chain lies in one sequence. Besides ba_chaining_create's
 * checks, every anchor must end at or before the end of the sequence that holds its start; the message names the problem and the anchor.
 * ba_chaining_reload keeps the table and the check. With one sequence the chains are ba_chaining_create's. */
BaChaining* ba_chaining_create_bounded(const struct BaChainingParams* params, const uint64_t* anchor_first, const uint32_t* q_anchor,
                                       const uint32_t* r_anchor, const uint32_t* anchor_len, uintptr_t n_problems, const uint64_t* seq_start,
                                       uintptr_t n_seqs);
/* Candidate windows of chains in an index's frame (host only). Chain c lies in sequence s, the one that holds its first anchor, from
 * S = seq_start[s] to E = seq_start[s + 1]; in 64-bit arithmetic lo = ra0 - min(ra0 - S, qa0 + margin), hi = re + min(E - re, (q_len - qe) +
 * margin); r_off_out = seq_off[s] + (lo - S), r_len_out = hi - lo, r_anchor_out = r_anchor - lo, seq_of_chain = s and local_shift = lo - S:
 * what to add to the chain batch's reference positions to get positions in sequence s. A chain without anchors, or with an anchor that
 * ends beyond E or beyond q_len, is refused with its number. Only seq_off says where a sequence lies in the pool. */
int ba_chain_windows_seqs(const uint32_t* q_len, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                          const uint32_t* anchor_len, uintptr_t n_chains, uint32_t margin, const uint64_t* seq_off, const uint32_t* seq_len,
                          uintptr_t n_seqs, uint64_t* r_off_out, uint32_t* r_len_out, uint32_t* r_anchor_out, uint32_t* seq_of_chain,
                          uint32_t* local_shift);
/* From the index's frame to a sequence (host only). For the closed interval [r_start, r_end], seq is the last non-empty sequence that
 * starts at or before r_start, local_start / local_end are the ends less seq_start[seq], and crosses says r_end > seq_start[seq + 1]: the
 * interval reaches into the next sequence. A position above seq_start[n_seqs], or r_end < r_start, is refused with the interval's number. */
int ba_ref_locate(const uint32_t* seq_len, uintptr_t n_seqs, const uint32_t* r_start, const uint32_t* r_end, uintptr_t n, uint32_t* seq,
                  uint32_t* local_start, uint32_t* local_end, uint8_t* crosses);

/* ---- both strands of a read at once: a canonical index ("Both strands at once": the rule, normative). The index of
 * ba_ref_index_create_multi -- the same arguments, checks and messages, the same sequence table, no k-mer and no window across a junction --
 * over canonical k-mers: a k-mer's code is the smaller of its own and its reverse complement's, its strand bit says whether that was the
 * reverse complement's, and a k-mer equal to its reverse complement is never selected. A key is code << 32 | strand << 31 | pos, so
 * ba_ref_index_entries on such an index returns pos with the strand in bit 31 (pos & 0x7fffffff is the position, pos >> 31 the strand),
 * ascending by (code, strand, position); longest_run counts a code's entries of both strands together. counts, sequences, times, destroy
 * and ba_ref_locate work unchanged. ba_seeding_create_indexed refuses such an index, and names ba_seeding_create_indexed_both. */
BaRefIndex* ba_ref_index_create_canonical(uint32_t k, uint32_t w, const uint8_t* pool, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs);
/* flag (or NULL): 1 for an index made by ba_ref_index_create_canonical, 0 for any other. */
int ba_ref_index_is_canonical(BaRefIndex* index, int* flag);
/* A seeder over n_reads reads (1 .. 2^27), each taken once: read r = pool[q_off[r] .. + q_len[r]) on strand s is problem 2 r + s of a
 * BaSeeding with 2 n_reads problems, and its hits are in the frame of ba_seeding_create_indexed's problem with that strand: r_hit in the
 * index's frame, q_hit in the oriented read. A read entry whose code more than max_occ of the read's entries have, or more than max_ref_occ
 * of the index's, gives no hits: both strands count together. The index must be canonical; a plain one is refused, and the message names
 * ba_seeding_create_indexed. The other arguments are checked before the index is looked at and before the device is touched. run, counts
 * (hits_per_problem: 2 n_reads entries), results (hit_first: 2 n_reads + 1), times, destroy and ba_chaining_create_seeded -- a chainer over
 * the 2 n_reads problems, bounded by the index's sequences -- work on the handle. ba_seeding_sketch gives per-read arrays: q_seed_first has
 * n_reads + 1 entries, q_seed_pos is in the read's own frame with the k-mer's strand in bit 31, q_seed_code is canonical, and there are no
 * reference entries (r_seed_first: n_reads + 1 zeros). More than 2^28 hits over all problems are refused with the read and the strand.
 * ba_seeding_reload and ba_seeding_reload_indexed refuse the handle, and ba_seeding_reload_indexed_both refuses any other seeder. */
BaSeeding* ba_seeding_create_indexed_both(BaRefIndex* index, uint32_t max_occ, uint32_t max_ref_occ, const uint8_t* pool, const uint64_t* q_off,
                                          const uint32_t* q_len, uintptr_t n_reads);
int ba_seeding_reload_indexed_both(BaSeeding* batch, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n_reads);
/* Any seeder's number of problems and of reads (either pointer may be NULL): 2 n_reads and n_reads for a both-strand seeder, n_problems
 * twice for any other. */
int ba_seeding_problems(BaSeeding* batch, uint64_t* n_problems, uint64_t* n_reads);

/* ---- read-level selection on the device: from candidates in any order -- chains before alignment, alignments after it -- to a mapper's
 * records: which of a read's candidates is primary, which are supplementary or secondary, which are dropped, and the mapping quality of the
 * heads ("Selecting a read's alignments": the rule, normative; all integer arithmetic, products in 64 bits).
 *
 * Candidate c belongs to read[c] < n_reads; the candidates of a read need be neither contiguous nor ordered, and a read may hold at most 1024.
 * It covers [q_start, q_end) of the oriented read, q_start <= q_end <= q_len (q_len: the read's length), on strand 0 or 1 (NULL: all 0); on
 * strand 1 its span in the read's own frame is [q_len - q_end, q_len - q_start). support (NULL: full support everywhere): what the mapping
 * quality is scaled by, such as a chain's anchors. exclude (NULL: none): non-zero takes the candidate out. A candidate that is excluded, scores
 * below min_score or has an empty span gets BA_SEL_EXCLUDED and plays no part. The others are ranked per read by score descending, index
 * ascending, and marked in that order: the first head (a primary or supplementary candidate so far, in rank order) that it overlaps by at
 * least mask_permille / 1000 of the shorter span is its parent, and it is secondary if it scores at least sec_permille / 1000 of the parent
 * and fewer than max_secondary secondaries of the read were kept, else dropped; without such a head it is a head itself, primary at rank 0,
 * supplementary otherwise. A head's mapq = mapq_max * (score - sub_score) * min(support, full_support) / (score * full_support), rounded
 * down, sub_score being the best score that hangs under it (0: none). Every argument is checked before the device is touched; a message
 * names the candidate, and for the cap the read. */
struct BaSelectParams {
    uint32_t mask_permille;   /* 1 .. 1000: the overlap with a head, of the shorter span, from which a candidate hangs under it */
    uint32_t sec_permille;    /* 0 .. 1000: a secondary scores at least this much of its parent */
    uint32_t max_secondary;   /* secondaries kept per read; 0 keeps none */
    uint32_t mapq_max;        /* 0 .. 255 */
    uint32_t full_support;    /* 1 .. 65535: the support from which the mapping quality is not scaled down */
    int32_t min_score;        /* >= 1: a candidate takes part from this score */
};
enum { BA_SEL_PRIMARY = 0, BA_SEL_SUPPLEMENTARY = 1, BA_SEL_SECONDARY = 2, BA_SEL_DROPPED = 3, BA_SEL_EXCLUDED = 4 };
typedef struct BaSelect BaSelect;
BaSelect* ba_select_create(const struct BaSelectParams* params, const uint32_t* read, const int32_t* score, const uint32_t* q_start,
                           const uint32_t* q_end, const uint32_t* q_len, const uint8_t* strand, const uint32_t* support, const uint8_t* exclude,
                           uintptr_t n, uintptr_t n_reads);
/* A selector over the results of a chain batch that has run: candidate c is the batch's chain c, of read read_of_chain[c]. score, q_start,
 * q_end and status are copied device to device from the batch's result buffers, q_len and strand are the batch's; a chain whose status has an
 * overflow, lost or watchdog bit (the bits after which ba_chain_batch_stats zeroes its record) is excluded. The batch need not have BA_TRACE.
 * Refused for a batch that has not finished a run since it was created or reloaded. The handle does not depend on the batch afterwards: the
 * copy is complete when the call returns. ba_select_reload refuses it. */
BaSelect* ba_select_create_chained(const struct BaSelectParams* params, BaChainBatch* ran, const uint32_t* read_of_chain, const uint32_t* support,
                                   uintptr_t n_reads);
/* Replace the candidates and keep parameters and device buffers: the new set must hold no more candidates and no more reads. */
int ba_select_reload(BaSelect* batch, const uint32_t* read, const int32_t* score, const uint32_t* q_start, const uint32_t* q_end, const uint32_t* q_len,
                     const uint8_t* strand, const uint32_t* support, const uint8_t* exclude, uintptr_t n, uintptr_t n_reads);
/* The grouping, the marking and the emit. kernels_ms (optional): the sum of their HIP-event times. */
int ba_select_run(BaSelect* batch, float* kernels_ms);
/* After a run: the candidates kept (class <= BA_SEL_SECONDARY) in all, and per read (n_reads entries). Either pointer may be NULL. */
int ba_select_counts(BaSelect* batch, uint64_t* n_kept, uint32_t* kept_per_read);
/* After a run, per candidate in the caller's order; any pointer may be NULL. cls: BA_SEL_*; mapq: heads only, else 0; parent: the head the
 * candidate hangs under (a head: itself); rank: its place among the read's eligible candidates; sub_score: heads only, else 0. An excluded
 * candidate has parent = rank = 0xffffffff. */
int ba_select_results(BaSelect* batch, uint8_t* cls, uint8_t* mapq, uint32_t* parent, uint32_t* rank, int32_t* sub_score);
/* After a run: what to report. kept_first (n_reads + 1 entries): where a read's kept candidates start; kept (n_kept entries): the candidates,
 * reads in order and in rank order within a read (the primary first). Either pointer may be NULL. */
int ba_select_kept(BaSelect* batch, uint64_t* kept_first, uint32_t* kept);
/* Device times of the last run in ms: the grouping's two passes with their scan, the marking with its scan, the emit. Any may be NULL. */
int ba_select_times(BaSelect* batch, float* group_ms, float* mark_ms, float* emit_ms);
void ba_select_destroy(BaSelect* batch);

/* ---- every pair with its own block range. The reference's callers choose the range per pair -- percent_len(max(|q|, |r|), 0.01) ..=
 * percent_len(max(|q|, |r|), p) in /root/reference/examples/nanopore_bench_global.rs:144-171, Block::align(..., min..=max, x) in
 * src/scan_block.rs:847 --, while ba_batch_create takes one range for the whole batch. These calls bin the pairs by (min, max), align every bin as
 * a batch of its own (same kernels, same results as ba_batch_create with that range) and give results and CIGAR runs back in the caller's order. */
typedef struct BaSizedBatch BaSizedBatch;
BaSizedBatch* ba_sized_batch_create(int kind, const void* matrix, struct Gaps gaps, const struct SizeRange* size_per_pair, int32_t x_drop, uint32_t mode,
                                    const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                    uintptr_t n_pairs);
/* ... the range of pair p = block_percent_len(max(|q|, |r|), min_percent) .. block_percent_len(max(|q|, |r|), max_percent) (lib.rs:109-111) */
BaSizedBatch* ba_sized_batch_create_percent(int kind, const void* matrix, struct Gaps gaps, float min_percent, float max_percent, int32_t x_drop, uint32_t mode,
                                            const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                            uintptr_t n_pairs);
/* The bins are launched together (each on its own stream, sharing the device) and waited for. kernel_ms (optional): host wall-clock milliseconds from the
 * first launch to the last completion -- overflow re-runs and the host's work between the waits included; NOT a sum of HIP-event times: the bins overlap
 * (per-bin event times of the same run: ba_sized_batch_classes).
 * A run that fails -- a wait past ba_set_wait_limit_ms above all, which leaves bins in flight or never launched -- leaves the SET without results:
 * ba_sized_batch_results, _cigars, _stats, _text, _exact* and _classes (returns -1) are refused until a later run completes for every bin. That
 * later run first waits, under the current limit, for every bin still in flight; if one is still running it fails with the same "did not finish
 * within ... still running" message and launches nothing, otherwise it runs all bins afresh. */
int ba_sized_batch_run(BaSizedBatch* batch, float* kernel_ms);
int ba_sized_batch_results(BaSizedBatch* batch, int32_t* score, uint32_t* query_idx, uint32_t* reference_idx, uint64_t* cells, uint32_t* cigar_len,
                           uint32_t* status);
int ba_sized_batch_cigars(BaSizedBatch* batch, uint32_t* runs, uint64_t capacity);
/* the bins: their ranges, pair counts, fill kernels (ba_batch_kernel) and kernel times of the last run; any pointer may be NULL; returns the number of bins */
int ba_sized_batch_classes(BaSizedBatch* batch, struct SizeRange* ranges, uint64_t* counts, int32_t* kernels, float* kernel_ms, int capacity);
void ba_sized_batch_destroy(BaSizedBatch* batch);

/* ---- one batch over several GPUs of a node (pairs are independent, so the batch shards without any exchange
 * step). The pair list is cut into contiguous cost-balanced slices (cost = |q| + |r|), one per entry of `devices` (an
 * entry may repeat a device); every slice is a batch of its own, built by its own host thread and launched on its own
 * stream. Results and CIGAR runs come back in the caller's pair order, exactly as from a single ba_batch_*. */
typedef struct BaMultiBatch BaMultiBatch;
BaMultiBatch* ba_multibatch_create(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, uint32_t mode,
                                   const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                                   const uint32_t* r_len, uintptr_t n_pairs, const int* devices, int n_devices);
/* Launch on every device, then wait for all. kernel_ms (optional) = the longest device's kernel time.
 * As ba_sized_batch_run: after a run that failed or timed out the set has no results -- ba_multibatch_results, _cigars, _stats, _text, _exact* and
 * _kernel_ms (returns -1) are refused --, and the next run first waits, under the current limit, for the slices still in flight (still running:
 * the same message, nothing launched), then runs every slice afresh. */
int ba_multibatch_run(BaMultiBatch* batch, float* kernel_ms);
int ba_multibatch_results(BaMultiBatch* batch, int32_t* score, uint32_t* query_idx, uint32_t* reference_idx, uint64_t* cells,
                          uint32_t* cigar_len, uint32_t* status);
int ba_multibatch_cigars(BaMultiBatch* batch, uint32_t* runs, uint64_t capacity);
/* slice boundaries: bounds[k] .. bounds[k + 1] are the pairs of devices[k]; returns the number of slices */
int ba_multibatch_parts(BaMultiBatch* batch, uint64_t* bounds, int capacity);
/* kernel time (ms, HIP events on the slice's own stream) of every slice in the last ba_multibatch_run; returns the number of slices */
int ba_multibatch_kernel_ms(BaMultiBatch* batch, float* ms, int capacity);
void ba_multibatch_destroy(BaMultiBatch* batch);
/* The slicing rule on its own (no device needed): bounds[0 .. parts] for contiguous slices of near-equal summed |q| + |r|. */
int ba_shard_slices(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n_pairs, int parts, uint64_t* bounds);

/* ---- per-alignment statistics, computed on the device from the CIGAR runs and the sequence images the fill left there (INTEGRATION.md,
 * "Alignment statistics"): what SAM (NM), BLAST tabular output (.m8) and parasail's *_stats report, and the start cell of the path.
 *
 * The batch must have been created with BA_TRACE and have finished a run (ba_batch_run, or ba_batch_launch + ba_batch_wait). Refused with a
 * message (ba_last_error) and a nonzero return: an untraced batch, a profile batch (its reference side has no bytes), a batch with a launch in
 * flight, a batch that never ran (or was reloaded since), a null argument.
 *
 * Match-type columns are M, = and X cells. "Equal" means equal image bytes, the rule of BA_CIGAR_EQ: for NucMatrix and AAMatrix batches the
 * converted bytes (lowercase input compares as uppercase), for ByteMatrix batches the raw bytes -- so matches / mismatches are the = / X cells
 * of the same batch run with BA_CIGAR_EQ. A pair without runs (X-drop stopped at once, an empty sequence) gets a record of zeros with
 * q_start = query_idx and r_start = reference_idx; a pair whose status has an overflow, lost or watchdog bit gets a record of zeros.
 * path_score equals the reported score in every mode but BA_FREE_QUERY_END_GAPS, whose reported score is the reference's (a vector lane of the
 * block's maximum, which need not belong to the end cell: block_aligner_amd/verify.py). The output buffer on the device is allocated on the
 * first call and freed by destroy. */
struct BaAlignStats {            /* 48 bytes, all 32-bit */
    uint32_t q_start, r_start;   /* first cell of the path: the end (query_idx / reference_idx) minus what the runs consume */
    uint32_t columns;            /* alignment columns: M/=/X + I + D cells */
    uint32_t matches;            /* match-type columns whose two image bytes are equal (exactly the cells BA_CIGAR_EQ calls '=') */
    uint32_t mismatches;         /* the other match-type columns */
    uint32_t positives;          /* match-type columns with matrix score > 0 (BLAST "positives", parasail "similar") */
    uint32_t ins, del;           /* I columns (query byte against a gap), D columns (reference byte against a gap) */
    uint32_t gap_opens;          /* I runs + D runs */
    uint32_t longest_ins, longest_del;
    int32_t  path_score;         /* the runs rescored: matrix over match-type columns + open + (n - 1) extend per gap run */
};
/* n_pairs records, in the caller's pair order */
int ba_batch_stats(BaBatch* batch, struct BaAlignStats* out);
int ba_sized_batch_stats(BaSizedBatch* batch, struct BaAlignStats* out);
int ba_multibatch_stats(BaMultiBatch* batch, struct BaAlignStats* out);
/* One record per seed, over q[q_start .. q_end) / r[r_start .. r_end) of the oriented query: the left side's record + the seed's ungapped
 * columns + the right side's record (counts add, the longest gaps are the larger; exact, since the joins only merge match-type runs);
 * q_start / r_start are the extension's. A seed whose status has a failure bit gets a record of zeros. */
int ba_extend_batch_stats(BaExtendBatch* batch, struct BaAlignStats* out);
/* One record per chain (n_chains records, the caller's order): the record of the chain's spliced runs -- those of ba_chain_batch_cigars --
 * over the oriented query (its reverse complement where strand[c] = 1) and the reference, ending at the chain's (q_end, r_end). Computed as
 * a sum over the chain's pieces: both ends' and every aligned gap's record, every anchor's ungapped columns, every gap with one empty slice
 * as one I or D run (counts add, the longest gaps are the larger). Exact: a gap run of one piece never merges with a gap run of another,
 * since an anchor lies between them. Hence q_start / r_start equal those of ba_chain_batch_results, path_score == score for every chain
 * with status 0, and matches + mismatches + ins + del == columns. A chain whose status has a failure bit gets a record of zeros.
 * Reference positions are in the frame of the r_off / r_len the batch was created with: the candidate window when the chains came through
 * ba_chain_windows (Python: chain_batch_args(margin=...)), whose `lo` (last_window_shift) brings them back to the reference's frame.
 * Refused as ba_extend_batch_stats is: a null batch, a null argument, a batch created without BA_TRACE, a batch that has not finished a
 * run (ba_chain_batch_run) since it was created or reloaded. */
int ba_chain_batch_stats(BaChainBatch* batch, struct BaAlignStats* out);
/* HIP-event times (ms) of the kernels the last ba_chain_batch_stats (the pieces' statistics and the combine) and the last
 * ba_chain_batch_text call on this batch ran; either pointer may be NULL. */
int ba_chain_batch_report_ms(BaChainBatch* batch, float* stats_ms, float* text_ms);
/* HIP-event time (ms) of the last ba_batch_stats kernel on this batch */
int ba_batch_stats_ms(BaBatch* batch, float* ms);

/* ---- exact full-matrix scores and the accuracy of the block heuristic ("Exact scores and accuracy").
 *
 * Block alignment is a heuristic; these calls compute, on the device, what a full |q| x |r| matrix gives for the same images, matrix and gaps,
 * so that a caller can count how often a block range misses the optimum on their own data. Scores are int32. A gap of length n costs
 * open + (n - 1) extend. Rows are query positions i = 0 .. |q|, columns reference positions j = 0 .. |r|, H[0][0] = 0, textbook Gotoh H / E / F.
 *   BA_EXACT_GLOBAL  H[|q|][|r|], reported with the end (|q|, |r|). An empty side gives the pure gap cost, two empty sides give 0.
 *   BA_EXACT_EXTEND  x_drop < 0: the maximum of H over every cell, cell (0, 0) = 0 included.
 *                    x_drop >= 0: rows are taken in order; rowmax_i = max over j of H[i][j] (row 0 includes cell (0, 0)), best = the largest
 *                    rowmax of the rows seen so far, row i included; after row i, if rowmax_i < best - x_drop, stop: later rows do not count.
 *                    Ties go to the smallest i, then the smallest j.
 *                    This is the row-wise rule of the scalar DP the reference's x_drop_accuracy example compares with, but for one point: there
 *                    cell (0, 0) is skipped, so a matrix without a positive cell yields a negative "best"; here the result is never below
 *                    0 at (0, 0), which is also what Block::<_, true> reports.
 * Two properties tie them to the batch results:
 *   - BA_EXACT_EXTEND with x_drop < 0 is an upper bound on the score of every BA_X_DROP batch over the same pair;
 *   - BA_EXACT_GLOBAL is an upper bound on the score of every batch without BA_X_DROP, and equals it when one block covers the matrix
 *     (min = max block size > max(|q|, |r|)).
 * rows = the query rows that counted: |q| + 1 unless the X-drop rule stopped earlier.
 *
 * which: pair indices in the caller's order, any order, repeats allowed; record k belongs to which[k]. NULL = every pair (n_which is ignored).
 * The calls need no prior run and no BA_TRACE: they read the images, the matrix and the gaps only, and change no result of a run.
 * Refused with a message (ba_last_error) and a nonzero return: a null batch, null out, an unknown `what`, an index out of range (the message
 * names it), a batch with a launch in flight, a profile batch, a batch with BA_LOCAL_START or BA_FREE_QUERY_*, a pair whose (|q| + |r|) * 128
 * does not stay above the minus-infinity sentinel -2^30 (the message names the pair), row buffers that do not fit device memory (the message
 * gives the bytes needed). A request is cut into kernel launches of a bounded number of cells. The device buffers are allocated on the first
 * call, grow, and are freed by destroy. */
enum { BA_EXACT_GLOBAL = 0, BA_EXACT_EXTEND = 1 };
struct BaExact {                 /* 16 bytes */
    int32_t  score;
    uint32_t query_idx, reference_idx;   /* the cell the score was read from */
    uint32_t rows;               /* query rows that counted */
};
int ba_batch_exact(BaBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out);
/* every part computes its own pairs (a multi-device batch: on its own device) */
int ba_sized_batch_exact(BaSizedBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out);
int ba_multibatch_exact(BaMultiBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out);
/* HIP-event time (ms) and cells (the sum of rows * (|r| + 1) over the request) of the last ba_batch_exact call on this batch; either may be NULL */
int ba_batch_exact_ms(BaBatch* batch, float* ms, uint64_t* cells);
/* BA_EXACT_EXTEND on both sides of every seed in `which` (seed indices; NULL = all), over the sides the batch already holds: left[k] is over
 * the reversed prefixes, right[k] over the suffixes, an empty side gives an all-zero record, and score[k] = left + the seed's ungapped score +
 * right: an upper bound (x_drop < 0) on the extension's own score. */
int ba_extend_batch_exact(BaExtendBatch* batch, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* left,
                          struct BaExact* right, int32_t* score);
/* The length guard of the exact calls on its own (host only, no device): nonzero, naming the pair, if a pair is too long for int32 scores. */
int ba_exact_check_lengths(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n_pairs);
/* ---- exact scores in the batch's own mode ("Exact scores and accuracy").
 *
 * BA_EXACT_OWN_MODE is a flag bit, OR-ed into BA_EXACT_GLOBAL or BA_EXACT_EXTEND in the `what` of ba_batch_exact, ba_sized_batch_exact and
 * ba_multibatch_exact. Without it every call is as described above, refusals included. With it on a plain sequence batch (none of
 * BA_LOCAL_START / BA_FREE_QUERY_*) the records are those without it. With it on a batch with one of those mode bits, or on a profile
 * batch (ba_batch_create_profile), the full matrix is computed under the batch's own start and end rules. Rows are query positions
 * i = 0 .. |q|, columns reference or profile positions j = 0 .. |r|, scores are int32; `rows` and the tie rules are as above.
 *
 * Sequence matrices. H, V (vertical gap) and Z (horizontal gap) are those above. The mode bits choose the start rule:
 *   none                      as above;
 *   BA_FREE_QUERY_START_GAPS  H[0][j] = 0 for every j; column 0 is as in the global case;
 *   BA_LOCAL_START            H[0][j] = H[i][0] = 0, and H[i][j] = max(0, H[i-1][j-1] + s(q_i, r_j), V[i][j], Z[i][j]).
 * (A batch cannot have both start bits; either goes with BA_FREE_QUERY_END_GAPS.) The quantity chooses the end rule:
 *   BA_EXACT_GLOBAL   H[|q|][|r|] -- in a BA_FREE_QUERY_END_GAPS batch instead the maximum over j = 0 .. |r| of H[|q|][j], ties to the
 *                     smallest j, reported at (|q|, j), with no floor at 0;
 *   BA_EXACT_EXTEND   as above: the maximum over every cell, row 0 included, under the row-wise X-drop rule when x_drop >= 0.
 *
 * Profile batches. Let e = gap_extend, oC[j], cC[j], oR[j] the profile's gap_open_C, gap_close_C and gap_open_R at position j = 0 .. |r|,
 * and s(j, a) the score of residue a at position j >= 1. Z is "no cell" in column 0, V in row 0, T[0][0] = 0 and T is "no cell" in the
 * rest of column 0:
 *   H[0][0] = 0
 *   Z[i][j] = max(H[i][j-1] + oC[j] + e, Z[i][j-1] + e)                         j >= 1, every i >= 0
 *   T[i][j] = max(H[i-1][j-1] + s(j, q_i) (i, j >= 1), Z[i][j] + cC[j] (j >= 1))
 *   V[i][j] = max(T[i-1][j] + oR[j] + e, V[i-1][j] + e)                         i >= 1, every j >= 0
 *   H[i][j] = max(T[i][j], V[i][j])
 * So a run of n profile positions j .. j+n-1 against no residue costs oC[j] + n e + cC[j+n-1], and a run of n residues after position j
 * costs oR[j] + n e. The vertical gap opens from T, as in the reference's prefix scan over the partially computed column; for oR <= 0
 * that coincides with opening from H. BA_EXACT_GLOBAL and BA_EXACT_EXTEND are read off this H as above (row 0 is a row like the others:
 * its maximum need not be cell (0, 0)). Positions the caller never set hold the reference's default of -128 and are taken as they are.
 *
 * What ties these to the batch results:
 *   - a batch without BA_X_DROP never scores above OWN_MODE BA_EXACT_GLOBAL of its own mode, and equals it when one block covers the
 *     matrix (min = max block size > max(|q|, |r|));
 *   - for a profile batch the bound needs gap costs that do not depend on the position (gap_open_C = gap_open_R, gap_close_C = 0, as
 *     the reference's pssm_accuracy example sets them). The definition is the recurrence of the rectangles whose vectors run along the
 *     query, the only kind when one block covers the matrix, where equality holds for any costs; the rectangles a smaller block range
 *     also places along the profile take the runs of profile positions through the prefix scan instead, which is another recurrence
 *     once the costs depend on the position, and a run of the reference can then score a few points above the definition's optimum
 *     (`above` of the summary);
 *   - a BA_X_DROP batch never scores above OWN_MODE BA_EXACT_EXTEND with x_drop < 0;
 *   - BA_FREE_QUERY_END_GAPS is the exception: the score a run reports follows the reference's lane rule -- the best of every block row
 *     whose index is |q| modulo 16, padded rows included, never below 0 -- and may exceed the exact value; path_score of ba_*_stats never
 *     does. For |q| < 16 with one block over the matrix the reported score equals max(exact, 0).
 *
 * Refused, beside the refusals above that do not concern the mode: BA_EXACT_OWN_MODE on a profile batch that also has BA_LOCAL_START or
 * BA_FREE_QUERY_* (that combination has no definition yet); BA_EXACT_OWN_MODE passed to ba_*_exact_cigars on a profile batch or a batch
 * with one of the mode bits (there the flag gives scores only; ba_*_exact_paths below returns those paths); a pair of a profile
 * batch whose (|q| + |r|) * 384 -- three int8 terms per column -- does not stay above the sentinel -2^30 (the message names the pair).
 * ba_extend_batch_exact has no `what`: extension batches are created without these modes and without profiles. */
enum { BA_EXACT_OWN_MODE = 1u << 8 };   /* OR-ed into BA_EXACT_GLOBAL / BA_EXACT_EXTEND */
/* The length guard of BA_EXACT_OWN_MODE on profile batches on its own (host only, no device): r_len are profile lengths. */
int ba_exact_check_lengths_profile(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n_pairs);
/* ---- optimal alignment paths of the exact full-matrix DP ("Exact scores and accuracy").
 *
 * The calls above say how far a block range is from the optimum; these return the optimum's alignment, as packed CIGAR runs of the traced
 * batches' format (length << 4 | op, ba_batch_cigars), for the same `what`, `x_drop` and `which`. The records are those of ba_*_exact.
 *
 * Definition. H is the matrix above. V[i][j] is the best score ending in a gap that consumes the query (CIGAR I), Z[i][j] the best score
 * ending in a gap that consumes the reference (D); for i, j >= 1
 *     V[i][j] = max(H[i-1][j] + open, V[i-1][j] + extend)        Z[i][j] = max(H[i][j-1] + open, Z[i][j-1] + extend)
 * and V and Z are "no cell" (minus infinity) in row 0 and column 0. The path ends at the record's cell (query_idx, reference_idx) -- (|q|, |r|)
 * for BA_EXACT_GLOBAL, the argmax under the tie rule above for BA_EXACT_EXTEND, with or without x_drop -- and starts at (0, 0). It is walked
 * backwards from the end cell, starting in state H:
 *   state H at (i, j):  i == 0: emit D x j and stop.  j == 0: emit I x i and stop.
 *                       else if H[i][j] == H[i-1][j-1] + s(q_i, r_j): emit one match-type column, go to (i-1, j-1), state H;
 *                       else if H[i][j] == V[i][j]: go to state V;  else: go to state Z.
 *   state V at (i, j):  emit I. If V[i][j] == V[i-1][j] + extend: go to (i-1, j), state V (extension is preferred); else to (i-1, j), state H.
 *   state Z at (i, j):  emit D. If Z[i][j] == Z[i][j-1] + extend: go to (i, j-1), state Z; else to (i, j-1), state H.
 * The runs are returned in alignment order, adjacent runs of one op merged (score-neutral: with open < extend the rule never closes and
 * reopens a gap at one cell, with open == extend the cost is linear). Match-type columns are M; in a BA_CIGAR_EQ batch they are = where the
 * two image bytes are equal and X elsewhere (the rule of the statistics' `matches`). A record with score 0 at (0, 0) has no runs, and so has
 * the record of an empty side in an extension batch's sense. Rescoring the runs (the matrix per match-type column, open + (n - 1) extend
 * per gap run) gives exactly `score`; they consume exactly query_idx query and reference_idx reference positions.
 *
 * Two-call pattern, as ba_batch_text: out (records) and run_off (records + 1 run offsets) are always filled. runs == NULL stops there; a runs
 * buffer of fewer than run_off[records] entries is refused with the count needed, the offsets still filled. A call with the arguments of the
 * one before it on the same batch, and no reload between them, copies what that call left on the device and computes nothing.
 *
 * Linear gap costs: ba_batch_create (and the sized and multi-device creates) accept open == extend for sequence matrices. Such a batch serves
 * ba_*_exact and ba_*_exact_cigars only: the block kernels, as the reference, need open < extend, and run / launch on it is refused with
 * "Gap open must cost more than gap extend!". Extension batches and the Block handles refuse open == extend as before.
 *
 * Refusals: those of ba_*_exact, null run_off, and a requested pair with |q| * |r| > BA_EXACT_TRACE_MAX_CELLS (the message names the pair). The
 * sweep keeps four bits per cell in a trace region per resident wave, sized for the largest requested pair (with the length limit above, below
 * 1.3 GiB); as many waves run at once as free device memory holds regions, one at least, and a request whose single region does not fit is
 * refused with the bytes needed. Every record's runs wait, unmerged with their neighbours' offsets, in 4 * (|q| + |r|) bytes until the offsets
 * are known. The buffers are allocated on the first call, grow, and are freed by destroy. Extension batches have no such call
 * (ba_extend_batch_exact_paths below is theirs). */
#define BA_EXACT_TRACE_MAX_CELLS 2147483648ull   /* 2^31 */
int ba_batch_exact_cigars(BaBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out,
                          uint64_t* run_off, uint32_t* runs, uint64_t capacity);
/* every part computes its own pairs (a multi-device batch: on its own device) */
int ba_sized_batch_exact_cigars(BaSizedBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out,
                                uint64_t* run_off, uint32_t* runs, uint64_t capacity);
int ba_multibatch_exact_cigars(BaMultiBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExact* out,
                               uint64_t* run_off, uint32_t* runs, uint64_t capacity);
/* HIP-event time (ms; sweep, walk, offsets and gather) and cells of the last ba_batch_exact_cigars call that computed; either may be NULL */
int ba_batch_exact_cigars_ms(BaBatch* batch, float* ms, uint64_t* cells);
/* The length guards of the path calls on their own (host only, no device): ba_exact_check_lengths' and |q| * |r| <= BA_EXACT_TRACE_MAX_CELLS. */
int ba_exact_trace_check_lengths(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n_pairs);
/* ---- optimal paths in the batch's own mode ("Optimal paths in the batch's own mode").
 *
 * ba_*_exact_cigars serve plain global-start sequence batches and refuse the rest; these calls return the optimal path of every batch a caller
 * can create: BA_LOCAL_START / BA_FREE_QUERY_* batches, profile batches, plain batches, and (ba_extend_batch_exact_paths) the seeds of an
 * extension batch. The older calls behave exactly as before.
 *
 * what: BA_EXACT_GLOBAL or BA_EXACT_EXTEND. The matrix is always that of the batch's own mode ("exact scores in the batch's own mode"
 * above); BA_EXACT_OWN_MODE may be OR-ed in and changes nothing. Any other quantity is refused.
 *
 * Records (struct BaExactPath): score, (q_end, r_end) and rows are what ba_*_exact(what | BA_EXACT_OWN_MODE) returns as score,
 * (query_idx, reference_idx) and rows; (q_start, r_start) is the cell where the walk below stopped. The runs (length << 4 | op, alignment
 * order, adjacent runs of one op merged) align q[q_start .. q_end) against r[r_start .. r_end): clipped ends produce no runs. Match-type
 * columns are M, or = / X by the image bytes in a BA_CIGAR_EQ sequence batch. A profile batch has no reference letters and emits M
 * (it cannot be created with BA_CIGAR_EQ: ba_batch_create_profile refuses the flag). Rescoring the runs from the start cell under the mode's rules gives exactly `score`.
 *
 * The walk, sequence matrices. H, V, Z are those of the own-mode score definition. The walk starts at the record's end cell in state H;
 * states V and Z are exactly those of ba_*_exact_cigars (extension preferred). State H at (i, j):
 *   BA_LOCAL_START            if H[i][j] == 0: stop. This comes before every move, a diagonal that also ties included; row 0 and column 0
 *                             are zero, so they stop too.
 *   BA_FREE_QUERY_START_GAPS  at i == 0: stop, emitting nothing. At j == 0: emit I x i and stop (at (0, 0)).
 *   neither start bit         (only BA_FREE_QUERY_END_GAPS, or a plain batch) at i == 0: emit D x j; at j == 0: emit I x i; stop at (0, 0).
 *   otherwise                 diagonal (one match-type column, to (i-1, j-1), state H) if H[i][j] == H[i-1][j-1] + s(q_i, r_j);
 *                             else state V if H[i][j] == V[i][j]; else state Z.
 * The end rule needs nothing of the walk: in a BA_FREE_QUERY_END_GAPS batch the BA_EXACT_GLOBAL record already ends at (|q|, argmax j).
 * On a plain batch the result equals ba_batch_exact_cigars run for run, with start (0, 0).
 *
 * The walk, profiles. T, Z, V, H are those of the profile recurrence above; row 0 is a row like the others. The walk starts in state H at
 * the end cell and always stops at (0, 0):
 *   state H at (i, j):  j == 0: emit I x i and stop. Otherwise go to state T if H[i][j] == T[i][j], else to state V.
 *   state T at (i, j):  (0, 0): stop. If i, j >= 1 and T[i][j] == H[i-1][j-1] + s(j, q_i): emit M, go to (i-1, j-1), state H.
 *                       Else go to state Z.
 *   state Z at (i, j):  emit D. If Z[i][j] == Z[i][j-1] + e stay in state Z, else go to state H; either way to (i, j-1).
 *   state V at (i, j):  emit I. If V[i][j] == V[i-1][j] + e stay in state V, else go to state T (V opens from T); either way to (i-1, j).
 * Four bits per cell suffice (H == T, T == diagonal, V extends, Z extends). Rescoring: a D run over positions j .. j+n-1 costs
 * oC[j] + n e + cC[j+n-1], an I run of n residues after position j costs oR[j] + n e, an M column s(j, q_i).
 *
 * Extension batches. Per requested seed the left side is walked over the reversed prefixes the batch holds, the right side over the suffixes,
 * both as ba_*_exact_cigars walks BA_EXACT_EXTEND. The runs are the left path turned round + the seed's ungapped columns (M, or = / X in a
 * BA_CIGAR_EQ batch) + the right path, merged across both joints. score = left + seed + right; q_start, r_start, q_end, r_end are in the
 * coordinates of ba_extend_batch_results (the oriented frame, for strand = 1 seeds too); rows = left.rows + right.rows; an empty side
 * contributes nothing. left / right (may be NULL) receive the sides' records as ba_extend_batch_exact gives them.
 *
 * Protocol and limits: the two-call pattern, the same-arguments cache, `which` and the memory and "in flight" refusals are those of
 * ba_batch_exact_cigars. BA_EXACT_TRACE_MAX_CELLS applies to |q| * |r|; a profile pair counts (|q| + 1) * |r|, because the profile sweep
 * owns row 0. The trace keeps four bits per cell (in a BA_LOCAL_START matrix "H == 0" is marked by the two bits the walk never reads
 * together), so the region size is that of ba_*_exact_cigars. Still refused: a profile batch that also has BA_LOCAL_START or
 * BA_FREE_QUERY_* -- its scores have no definition either. */
struct BaExactPath { int32_t score; uint32_t q_start, r_start, q_end, r_end, rows; };   /* 24 bytes */
int ba_batch_exact_paths(BaBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExactPath* out,
                         uint64_t* run_off, uint32_t* runs, uintptr_t runs_cap);
/* every part computes its own pairs (a multi-device batch: on its own device) */
int ba_sized_batch_exact_paths(BaSizedBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExactPath* out,
                               uint64_t* run_off, uint32_t* runs, uintptr_t runs_cap);
int ba_multibatch_exact_paths(BaMultiBatch* batch, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExactPath* out,
                              uint64_t* run_off, uint32_t* runs, uintptr_t runs_cap);
int ba_extend_batch_exact_paths(BaExtendBatch* batch, int32_t x_drop, const uint32_t* which, uintptr_t n_which, struct BaExactPath* out,
                                struct BaExact* left, struct BaExact* right, uint64_t* run_off, uint32_t* runs, uintptr_t runs_cap);
/* HIP-event time (ms; sweep, walk, offsets and gather) and cells of the last ba_batch_exact_paths call that computed; either may be NULL */
int ba_batch_exact_paths_ms(BaBatch* batch, float* ms, uint64_t* cells);
/* The length guards of the path calls on a profile batch on their own (host only, no device): ba_exact_check_lengths_profile's and
 * (|q| + 1) * |r| <= BA_EXACT_TRACE_MAX_CELLS. For sequence batches ba_exact_trace_check_lengths holds. */
int ba_exact_paths_check_lengths_profile(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n_pairs);
/* Host only, no device: the results of a run against exact records of the same pairs. Pairs whose status has an overflow, lost or watchdog
 * bit are skipped; diff = exact - score over the others; wrong counts diff != 0, below diff > 0 (the heuristic missed the optimum), above
 * diff < 0; diff_end counts compared pairs whose end cell differs; mean_rel_error is the mean of diff / |exact| over the wrong pairs with
 * exact != 0 (0 if there are none); min_diff / max_diff range over the wrong pairs (0 when nothing is wrong). query_idx, reference_idx and
 * status may be NULL (no end comparison / nothing skipped). */
struct BaAccuracy {
    uint64_t n, compared, skipped, wrong, below, above, diff_end;
    double   mean_rel_error;
    int32_t  min_diff, max_diff;
};
int ba_accuracy_summary(const int32_t* score, const uint32_t* query_idx, const uint32_t* reference_idx, const uint32_t* status,
                        const struct BaExact* exact, uintptr_t n, struct BaAccuracy* out);

/* ---- alignment strings, rendered on the device from the CIGAR runs and the sequences the fill left there ("Alignment
 * strings"): the CIGAR (optionally soft-clipped), the SAM MD:Z value and minimap2's short cs:Z value of every traced alignment, in one text
 * buffer per call.
 *
 * An alignment is its runs in alignment order (ba_*_cigars) from its first cell (q_start, r_start of ba_*_stats). The letters are those of
 * the image bytes: uppercase for NucMatrix, 'A' + code for AAMatrix, and for extension batches the oriented query (the reverse complement
 * on the minus strand). "Equal" is BA_CIGAR_EQ's rule.
 *   BA_TEXT_CIGAR  <len><op> per run (M = X I D): byte for byte the runs' string. | BA_TEXT_SOFT_CLIP: <q_start>S in front when q_start > 0,
 *                  <q_len - q_end>S behind when that is > 0 (q_end = query_idx; for extension batches the result's q_end over the whole
 *                  query). Every traced batch, profile and ByteMatrix batches included.
 *   BA_TEXT_MD     SAM MD:Z without the prefix: equal match-type columns count, a mismatch emits the count and the reference letter, a D run
 *                  the count, '^' and its reference letters; I columns emit nothing and do not break the count; the count closes it. Always
 *                  [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.
 *   BA_TEXT_CS     minimap2's short cs:Z without the prefix: :<n> per stretch of equal columns, *<ref><query> per mismatch, +<query> per I run,
 *                  -<ref> per D run, letters lowercase; an I run ends a stretch.
 * A pair without runs, or whose status has an overflow, lost or watchdog bit, gets empty text (SAM / PAF: '*').
 *
 * offsets: n_pairs + 1 entries, the caller's pair order, offsets[0] = 0; pair p's text is text[offsets[p] .. offsets[p + 1]), no terminators.
 * text == NULL: fill offsets only. text != NULL and capacity < offsets[n_pairs]: refused with the bytes needed (the offsets are filled).
 * The second call of that pattern (same `what`, same run) reuses the sizes on the device and only renders.
 *
 * Refused with a message (ba_last_error) and a nonzero return as the stats calls are (untraced, a launch in flight, never ran or reloaded
 * since, a null batch, null offsets), and: MD or cs on a ByteMatrix batch (raw bytes need not be letters) or a profile batch (no reference
 * letters), BA_TEXT_SOFT_CLIP with MD or cs, an unknown `what`. The device buffers are allocated on the first call, grow, and are freed by
 * destroy. */
enum { BA_TEXT_CIGAR = 0, BA_TEXT_MD = 1, BA_TEXT_CS = 2, BA_TEXT_SOFT_CLIP = 1u << 8 };
int ba_batch_text(BaBatch* batch, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity);
int ba_sized_batch_text(BaSizedBatch* batch, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity);
int ba_multibatch_text(BaMultiBatch* batch, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity);
int ba_extend_batch_text(BaExtendBatch* batch, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity);
/* Chain c's text: its spliced runs (ba_chain_batch_cigars) from (q_start, r_start) over the oriented query and the reference, as for an
 * extension batch; BA_TEXT_SOFT_CLIP clips over the oriented query's full length. n_chains + 1 offsets, the two-call pattern above. A chain
 * whose status has a failure bit gets empty text. Reference letters and positions are those of the r_off / r_len the batch was created with
 * (the candidate window after ba_chain_windows). Refused as ba_extend_batch_text is. */
int ba_chain_batch_text(BaChainBatch* batch, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity);
/* HIP-event time (ms) of the text kernels the last ba_batch_text call on this batch ran (the sizes, the rendering, or both) */
int ba_batch_text_ms(BaBatch* batch, float* ms);

enum { BA_ST_TRACE_OVERFLOW = 1, BA_ST_BLOCKS_OVERFLOW = 2, BA_ST_CIGAR_OVERFLOW = 4, BA_ST_TRACEBACK_LOST = 8, BA_ST_WATCHDOG = 16,
       BA_ST_SLOT_TIMEOUT = 32 /* never reported since round 4 (a fill wave that waits for a trace slot walks pending tracebacks itself); kept for ABI stability */,
       BA_ST_MODE = 64 /* FREE_QUERY_END_GAPS reached a down step: the reference panics there */ };
/* (bit 128 is the library's own: a pair of a block range that ends above 2048 cells wanted to grow past the 2048-cell class its batch was launched in -- ba_batch_wait
 * runs such pairs again in the row-tiled class before it returns, so the bit is never reported) */

/* One-shot convenience over create/run/results/cigars/destroy. */
int block_batch_align(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, uint32_t mode,
                      const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                      const uint32_t* r_len, uintptr_t n_pairs, struct AlignResult* results, uint32_t* cigar_runs,
                      uint64_t cigar_capacity, uint32_t* cigar_len);

/* Block::align_exp / align_profile_exp over a batch (scan_block.rs:884-902, 974-992): every pair is aligned with the min
 * block size size.min; the pairs whose score stays below target_score go through another kernel pass with the min size
 * doubled, until they reach the target or the min size would exceed size.max. reached_min[p] = the min block size at
 * which pair p reached the target, 0 if it never did (results[p] is then that of the last attempt, as in the reference).
 * Scores and end positions only: BA_TRACE / BA_CIGAR_EQ are ignored (trace the finished pairs with ba_batch_create). */
int block_batch_align_exp(int kind, const void* matrix, struct Gaps gaps, struct SizeRange size, int32_t x_drop, int32_t target_score,
                          uint32_t mode, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                          const uint32_t* r_len, uintptr_t n_pairs, struct AlignResult* results, uintptr_t* reached_min);
int block_batch_align_profile_exp(const struct AAProfile* const* profiles, struct SizeRange size, int32_t x_drop, int32_t target_score,
                                  uint32_t mode, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n_pairs,
                                  struct AlignResult* results, uintptr_t* reached_min);

#ifdef __cplusplus
}
#endif
#endif /* BLOCK_ALIGNER_HIP_H */
