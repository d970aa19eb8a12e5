// block_aligner_amd — host side of the C ABI declared in include/block_aligner_hip.h.
// Owns device memory, builds PaddedBytes images, launches the gfx950 kernels (ba_kernels.hip) and mirrors the
// reference's ffi.rs objects (PaddedBytes, AAMatrix, AAProfile, Cigar, Block handles). No alignment arithmetic is
// done on the host: without a usable HIP device every align call fails (batch API: error code; reference API: abort).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <atomic>
#include <chrono>
#include <thread>

#include "../../include/block_aligner_hip.h"
#include "aa_matrices.inc"
#include "ba_launch.h"

using ba::BatchParams;
using ba::BlockRec;

// ------------------------------------------------------------------ the kernel catalogue (ba_launch.h)
// [special modes?][kind][block class][family]: filled by the kernel translation units while the library loads.
typedef const ba::KernelEntry* KernelTable[2][ba::N_KINDS][ba::N_CLASSES][ba::FAM_COUNT];
static KernelTable& kernel_table() { static KernelTable t = {}; return t; }
int ba::register_kernels(int kind, int pmax, bool special, const ba::KernelEntry* entries, int n) {
    int pc = 0;
    while ((1 << pc) < pmax) pc++;   // packed registers per lane 1 .. 16 -> block class 0 .. 4, 32 -> the row-tiled class
    for (int k = 0; k < n; k++) kernel_table()[special][kind][pc][entries[k].family] = &entries[k];
    return n;
}
static const ba::KernelEntry* find_kernel(int family, int kind, int pc, int special) {
    if (family < 0 || family >= ba::FAM_COUNT || kind < 0 || kind >= ba::N_KINDS || pc < 0 || pc >= ba::N_CLASSES || special < 0 || special > 1) return nullptr;
    return kernel_table()[special][kind][pc][family];
}
constexpr int BA_PCLASS_BIG = 5;
static inline int special_of(uint32_t mode) { return (mode & (BA_LOCAL_START | BA_FREE_QUERY_START_GAPS | BA_FREE_QUERY_END_GAPS)) ? 1 : 0; }
constexpr int BA_KIND_PROFILE_ = ba::KIND_PROFILE;   // batches whose "reference" is an AAProfile (sequence bytes: AA alphabet)

// ------------------------------------------------------------------ development switches
// The release library reads NO environment variables: its results and its launch geometry depend on the call's arguments only.
// Built with -DBA_DEV (lib/libblock_aligner_hip_dev.so: the tests that force a code path on small inputs, the measurement
// scripts under tools/) the switches below exist; they are listed in README.md.
#ifdef BA_DEV
#define dev_env(name) getenv(name)
#else
#define dev_env(name) ((const char*)nullptr)
#endif
#ifndef BA_BUILD_ID
#define BA_BUILD_ID "unknown"
#endif
extern "C" const char* ba_build_id(void) { return BA_BUILD_ID; }   // tools/kernel_hash.py over the kernel sources at build time
extern "C" int ba_dev_build(void) {
#ifdef BA_DEV
    return 1;
#else
    return 0;
#endif
}

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return 1;
}
[[noreturn]] static void die(const char* fmt, ...) {   // reference contract: assert! -> panic = abort (Cargo.toml:41)
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fprintf(stderr, "block_aligner_hip: %s\n", buf);
    abort();
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

static thread_local int g_device = -1;   // per host thread: one thread may drive each GPU (ba_set_device; BaMultiBatch does)
static int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail("no usable HIP device (hipGetDeviceCount: %s); block_aligner_hip has no CPU fallback", hipGetErrorString(e));
    if (g_device < 0) g_device = 0;
    HIP_TRY(hipSetDevice(g_device));
    return 0;
}

// ------------------------------------------------------------------ matrices (layouts fixed by the reference ABI)
struct AAMatrix { alignas(32) int8_t scores[27 * 32]; };
struct NucMatrix { alignas(32) int8_t scores[8 * 16]; };

static constexpr AAMatrix expand_tri(const signed char* tri) {
    AAMatrix m{};
    for (int k = 0; k < 27 * 32; k++) m.scores[k] = -128;
    int idx = 0;
    const char* letters = BA_AA_LETTERS;
    for (int a = 0; a < BA_AA_NLETTERS; a++)
        for (int b = 0; b <= a; b++) {
            const int ia = letters[a] - 'A', ib = letters[b] - 'A';
            m.scores[ia * 32 + ib] = tri[idx];
            m.scores[ib * 32 + ia] = tri[idx];
            idx++;
        }
    return m;
}
static constexpr NucMatrix nuc_simple(int8_t match, int8_t mismatch) {   // scores.rs:150-164
    NucMatrix m{};
    for (int k = 0; k < 8 * 16; k++) m.scores[k] = -128;
    const char alpha[5] = {'A', 'T', 'C', 'G', 'N'};
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) m.scores[(alpha[i] & 7) * 16 + (alpha[j] & 15)] = i == j ? match : mismatch;
    return m;
}
extern "C" {
extern const NucMatrix NW1 = nuc_simple(1, -1);
extern const AAMatrix BLOSUM45 = expand_tri(BA_TRI_BLOSUM45);
extern const AAMatrix BLOSUM50 = expand_tri(BA_TRI_BLOSUM50);
extern const AAMatrix BLOSUM62 = expand_tri(BA_TRI_BLOSUM62);
extern const AAMatrix BLOSUM80 = expand_tri(BA_TRI_BLOSUM80);
extern const AAMatrix BLOSUM90 = expand_tri(BA_TRI_BLOSUM90);
extern const AAMatrix PAM100 = expand_tri(BA_TRI_PAM100);
extern const AAMatrix PAM120 = expand_tri(BA_TRI_PAM120);
extern const AAMatrix PAM160 = expand_tri(BA_TRI_PAM160);
extern const AAMatrix PAM200 = expand_tri(BA_TRI_PAM200);
extern const AAMatrix PAM250 = expand_tri(BA_TRI_PAM250);
extern const ByteMatrix BYTES1 = {1, -1};
}

static inline uint8_t upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
static inline int seq_kind(int kind) { return kind == BA_KIND_PROFILE_ ? BA_KIND_AA : kind; }
static inline uint8_t null_byte(int kind) { kind = seq_kind(kind); return kind == BA_KIND_AA ? 26 : (kind == BA_KIND_NUC ? 'Z' : 0); }
// convert_char of scores.rs:130-134 / 212-216 / 270-272; returns false on a byte the reference would assert on
static inline bool convert_char(int kind, uint8_t c, uint8_t* out) {
    kind = seq_kind(kind);
    if (kind == BA_KIND_BYTES) { *out = c; return true; }
    c = upper(c);
    if (kind == BA_KIND_AA) { if (c < 'A' || c > 'A' + 26) return false; *out = (uint8_t)(c - 'A'); return true; }
    if (c < 'A' || c > 'Z') return false;
    *out = c;
    return true;
}

// ------------------------------------------------------------------ host mirrors of the reference's opaque objects
struct PaddedBytes {   // scan_block.rs:1790-1884
    std::vector<uint8_t> s;
    size_t len;
    int kind;
};
struct Cigar {         // cigar.rs:42-145; runs kept in alignment order
    std::vector<OpLen> ops;
    size_t capacity;   // query_len + reference_len + 5 (cigar.rs:50)
};
struct AAProfile {     // scores.rs:452-468
    std::vector<int8_t> pos_aa;                    // [curr_len][32]
    std::vector<int16_t> gap_open_C, gap_close_C, gap_open_R;
    int8_t gap_extend;
    size_t max_len, curr_len, str_len;
};

// ------------------------------------------------------------------ device batch
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool owned = true;
    void view(void* q, size_t n) { free_(); p = q; bytes = n; owned = false; }   // a window into another buffer
    int alloc(size_t n) {
        free_();
        owned = true;
        if (n == 0) n = 4;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return fail("hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e)); }
        bytes = n;
        return 0;
    }
    void free_() { if (p && owned) (void)hipFree(p); p = nullptr; bytes = 0; }
    ~DevBuf() { free_(); }
    template <class T> T* as() const { return (T*)p; }
};

// Alignment strings (ba_*_text) of one batch: per-pair sizes in the caller's order, their offsets, the device -> caller position map and the
// text, allocated on the first call (the text buffer grows, never shrinks) and freed with the batch. The sizes are kept for the run and the
// format they were computed for: the second call of the two-call pattern only renders. ms: the kernels of the last call.
struct TextState {
    DevBuf len, off, pos, buf;
    uint64_t buf_cap = 0, run = 0;
    uint32_t what = ~0u;
    bool sized = false;
    hipEvent_t ev[2] = {};
    float ms = 0;
    ~TextState() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

struct BaBatch {
    int device = 0;
    hipStream_t stream = nullptr, stream2 = nullptr;   // stream2: pair-slot small-block batches (see batch_launch)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join = nullptr, ev_l0 = nullptr, ev_m1 = nullptr;   // ev_l0 / ev_m1: batch_retry
    int kind = 0; uint32_t mode = 0;
    uint32_t n = 0, min_size = 0, max_size = 0, pclass = 0;
    int gap_open = 0, gap_extend = 0, x_drop = 0;
    uint32_t grid = 0, lds = 0, slots = 0;   // grid = workgroups of WAVES_PER_WG waves; slots = resident waves
    uint64_t trace_stride = 0, blocks_stride = 0, cig_total = 0, pool_bytes = 0;
    uint64_t trace_full = 0;    // trace words per slot by the reference's worst-case bound (Trace::new)
    bool adaptive = false;      // trace_stride < trace_full: pairs that overflow their slot are re-run by batch_wait
    bool opt_class = false;     // round 6: max_size belongs to the row-tiled class, the launch is the 2048-cell class's; pairs whose block wants past 2048 cells are re-run by batch_wait
    bool bet_lost = false;      // ... and the last run re-ran more than an eighth of its pairs: the next launch is the row-tiled class's (batch_drop_class_bet)
    uint64_t plan_fixed = 0, plan_maxlen2 = 0, plan_avg = 0;   // batch_plan's arguments, for that second plan
    uint32_t retried = 0;       // pairs the last run had to re-run with full-size slots
    uint64_t cap_n = 0, cap_pool = 0, cap_cig = 0, cap_maxlen2 = 0;   // what the device buffers were sized for (ba_batch_reload)
    DevBuf pool, q_off, q_len, r_off, r_len, matrix, score, qidx, ridx, cig_ops, cig_off, cig_len, cells, status, nblocks, pair_slot, trace_words, trace, blocks, ckpt, big, counter,
           tb_queue, tb_ctrl, slot_free, slot_info, prof, params_dev, donate;
    std::vector<uint32_t> h_order;   // device order -> caller's pair index (empty: identical); see Packed::order
    uint32_t tb_stride = 0, n_fill_waves = 0, slots_per_wave = 1, tb_qsize = 1, tb_reserve = 0;
    std::vector<uint64_t> h_q_off, h_r_off;   // padded offsets (host copy, for the per-handle traceback)
    bool ran = false, in_flight = false;
    uint32_t work_chunk = 1;    // pairs a wave takes per work-counter atomic (short pairs outrun one counter's ~90 atomics / us)
    uint32_t mq_drain = 0;      // k_multi: pairs at the end of the batch that are run one at a time (BatchParams::mq_drain)
    bool multi = false;         // the batch starts at 128 cells: four pairs per wave while a pair's block is 128 cells (ba_multi.hpp)
    uint32_t multi_b = 128;     // ... or at 256 cells (round 6): two pairs per wave, slots of 32 lanes
    uint32_t geom = 0;          // k_multi, round 6: 0 = workgroups of WAVES_PER_WG waves at four waves per SIMD; 3 / 2 = four-wave workgroups at that many waves per SIMD (batch_build)
    uint32_t wpw = ba::WAVES_PER_WG;   // waves per workgroup of the batch's launch (MQ_GEOM_WPW with geom)
    uint32_t walk_wave_n = 0;   // k_walk: the first walk_wave_n pairs of the batch order are walked one to a wave (plan_walks)
    uint32_t sm_excl_n = 0;     // k_small: the batch's longest pairs, run one to a wave (plan_exclusive)
    uint32_t sm_side_n = 0;     // ... of which the first sm_side_n run in a launch of their own beside the main one (TRACE batches: batch_launch)
    bool small = false;         // small-block batch: sixteen pairs per wave while their block is 32 cells, everything else by the same wave (ba_small.hpp)
    bool quad = false;          // small-block batch: pairs run 4 per wave while their block is 32 cells (ba_quad.hpp)
    DevBuf contA, cont_n;       // the PairCont records of the pairs k_quad hands to the per-pair kernel, and the per-pair flags
    DevBuf cq_queue, cq_ctrl;   // the queue those pairs travel through (ba_params.h)
    uint32_t quad_grid = 0, cq_grid = 0;   // workgroups of k_quad / of the per-pair kernel that runs beside it
    // pair-slot batch (a small-block batch with TRACE): every pair owns a region of the trace / record arenas for the whole
    // batch (offsets below, n + 1 entries each), the fill kernels only stack, and k_walk does all tracebacks at the end
    bool pipe = false;
    DevBuf trace_off, blocks_off;
    uint64_t pipe_words = 0, pipe_recs = 0;   // arena capacities (ba_batch_reload re-cuts them)
    // CIGAR runs gathered on the device right behind the alignment kernels (ba_batch_compact_cigars): the later ba_batch_cigars is then one
    // device-to-host copy -- no kernel that would have to wait for room beside another batch's persistent launch
    DevBuf compact, compact_off, compact_total, dev_of;
    // per-alignment statistics (ba_batch_stats): the records and the device -> caller position map, allocated on the first call; the kernel's time
    DevBuf stats, stats_pos;
    hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr;
    float stats_ms = 0;
    // exact full-matrix scores (ba_batch_exact): the waves' row buffers, the sorted request, its records and one work counter per launch,
    // allocated on the first call (they grow, never shrink); time and cells of the last call
    DevBuf ex_rows, ex_work, ex_out, ex_counter;
    hipEvent_t ev_x0 = nullptr, ev_x1 = nullptr;
    float exact_ms = 0; uint64_t exact_cells = 0;
    // optimal paths (ba_batch_exact_cigars): the waves' trace regions, every record's reversed runs and where they start, the run counts,
    // their offsets and the run array, allocated on the first call (they grow, never shrink). The request whose records, offsets and runs
    // they hold is kept, so that the second call of the two-call pattern only copies.
    DevBuf xt_trace, xt_rev, xt_rev_off, xt_nrun, xt_off, xt_runs;
    float xt_ms = 0; uint64_t xt_cells = 0;
    bool xt_valid = false; uint32_t xt_what = 0; int32_t xt_x_drop = 0; uint64_t xt_loads = 0;
    std::vector<uint32_t> xt_devpos; std::vector<BaExact> xt_out; std::vector<uint64_t> xt_h_off;
    // ... shared with the paths of the batch's own mode (ba_batch_exact_paths), which add every record's start cell; xt_form says whose
    // request the buffers hold (EXACT_FORM_*)
    int xt_form = 0;
    float xp_ms = 0; uint64_t xp_cells = 0;   // time and cells of the last ba_batch_exact_paths call that computed
    DevBuf xt_start; std::vector<uint32_t> xt_h_start;
    uint64_t loads = 0;      // reloads so far
    TextState text;          // alignment strings (ba_batch_text)
    uint64_t runs_done = 0;  // finished runs: what the text sizes are kept for
    uint64_t compact_cap = 0, compact_used_cap = 0; bool compacted = false; uint32_t* compact_host = nullptr;
    unsigned long long* h_total = nullptr;   // page-locked mailbox the gather writes its total to (read without a copy)
    bool pad_negative = false;  // every matrix entry of the padding byte's row and column is negative (pad_negative() at creation): the kernels may clip an X-drop alignment's last block (F_PAD_NEG)
    bool handle_mode = false;   // the device state of one Block handle: one pair per launch, CIGARs only on request (k_traceback)
    DevBuf hblk, rblk;          // handle mode: everything uploaded per align / everything read back, one buffer each
    // a sequence offset of k_multi's prefetch (pool + two blocks + 8 bytes) could pass 32 bits, or BA_POOL64 in the development library: traced
    // k_multi batches run the kernels that fetch by 64-bit offset (kernel_fn)
    bool pool64() const { return (uint64_t)pool.bytes + 2ull * max_size + 8ull > 0xffffffffull || dev_env("BA_POOL64"); }
    BatchParams params() const {
        BatchParams bp{};
        bp.pool = pool.as<uint8_t>();
        bp.q_off = q_off.as<uint64_t>(); bp.q_len = q_len.as<uint32_t>();
        bp.r_off = r_off.as<uint64_t>(); bp.r_len = r_len.as<uint32_t>();
        bp.n = n; bp.gap_open = gap_open; bp.gap_extend = gap_extend;
        bp.min_size = min_size; bp.max_size = max_size; bp.x_drop = x_drop; bp.flags = mode | (dev_env("BA_NO_FAST") ? 0x100u : 0u) | ((dev_env("BA_SKIP_WALK") || dev_env("BA_NO_TRACEBACK")) ? 0x200u : 0u) | ((handle_mode || dev_env("BA_NO_SPEC")) ? 0x400u : 0u) | (dev_env("BA_NO_TB_WAVES") ? 0x800u : 0u) | (dev_env("BA_NO_REFILL") ? 0x1000u : 0u) | (dev_env("BA_NO_STEAL") ? 0x2000u : 0u) | ((pad_negative && !dev_env("BA_NO_END_CLIP")) ? (uint32_t)ba::F_PAD_NEG : 0u) | (pool64() ? (uint32_t)ba::F_POOL64 : 0u) | (dev_env("BA_COUNT_STEPS") ? (uint32_t)ba::F_COUNT_STEPS : 0u);   // (0x400: no speculative grows -- a handle's trace may be walked from any cell)
        bp.matrix = matrix.as<int8_t>();
        bp.score = score.as<int32_t>(); bp.query_idx = qidx.as<uint32_t>(); bp.reference_idx = ridx.as<uint32_t>();
        bp.cig_ops = ((mode & BA_TRACE) && !handle_mode && !dev_env("BA_NO_TRACEBACK")) ? cig_ops.as<uint32_t>() : nullptr;   // env: development switch
        bp.cig_off = cig_off.as<uint64_t>(); bp.cig_start = nullptr; bp.cig_len = cig_len.as<uint32_t>();
        bp.cells = cells.as<unsigned long long>(); bp.status = status.as<uint32_t>(); bp.nblocks_out = nblocks.as<uint32_t>(); bp.slot_out = pair_slot.as<uint32_t>(); bp.trace_words_out = trace_words.as<uint32_t>();
        bp.walk_wave_n = walk_wave_n;
        bp.trace_arena = trace.as<uint32_t>(); bp.trace_stride = trace_stride;
        bp.blocks = blocks.as<BlockRec>(); bp.blocks_stride = blocks_stride;
        bp.trace_off = pipe ? trace_off.as<uint64_t>() : nullptr; bp.blocks_off = pipe ? blocks_off.as<uint64_t>() : nullptr;
        bp.ckpt = ckpt.as<short>(); bp.big = big.as<short>();
        bp.tb_stride = tb_stride; bp.slots_per_wave = slots_per_wave; bp.n_slots = slots; bp.tb_reserve = tb_reserve;
        bp.tb_qmask = tb_qsize - 1;
        bp.tb_queue = tb_queue.as<uint32_t>(); bp.tb_ctrl = tb_ctrl.as<uint32_t>();
        bp.slot_free = slot_free.as<uint32_t>(); bp.slot_info = slot_info.as<ba::SlotInfo>();
        bp.work_counter = counter.as<uint32_t>();
        bp.work_chunk = work_chunk;
        bp.mq_drain = mq_drain;
        bp.mq_waves = grid * wpw;
        bp.mq_donate = (multi && (mode & BA_TRACE) && !special_of(mode) && donate.p && !dev_env("BA_NO_DONATE")) ? donate.as<uint32_t>() : nullptr;   // (the special modes: no slot donation)   // (the score-only kernels are compiled without the end-of-batch code)
        bp.sm_excl_n = small ? sm_excl_n : 0; bp.sm_excl_first = 0;
        bp.prof = prof.as<unsigned long long>();
        return bp;
    }
    ~BaBatch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (h_total) (void)hipHostFree(h_total);
        if (ev_l0) (void)hipEventDestroy(ev_l0);
        if (ev_m1) (void)hipEventDestroy(ev_m1);
        if (ev_s0) (void)hipEventDestroy(ev_s0);
        if (ev_s1) (void)hipEventDestroy(ev_s1);
        if (ev_x0) (void)hipEventDestroy(ev_x0);
        if (ev_x1) (void)hipEventDestroy(ev_x1);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// linear_ok: open == extend passes (batch_build: such a batch serves the exact calls only, batch_launch refuses it)
static int check_align_params(bool profile, Gaps g, size_t min_size, size_t max_size, int32_t x_drop, uint32_t mode, std::string* why, bool linear_ok = false) {
    // scan_block.rs:847-862 (align) / 942-956 (align_profile: only the extend cost, which lives in the profile)
    if (profile) { if (!(g.extend < 0)) { *why = "Gap extend cost must be negative!"; return 1; } }
    else {
        if (!(g.open < 0 && g.extend < 0)) { *why = "Gap costs must be negative!"; return 1; }
        if (!(g.open < g.extend) && !(linear_ok && g.open == g.extend)) { *why = "Gap open must cost more than gap extend!"; return 1; }
    }
    if (!(min_size < 65535 && max_size < 65535)) { *why = "Block sizes must be smaller than 2^16 - 1!"; return 1; }
    if ((min_size & (min_size - 1)) || (max_size & (max_size - 1))) { *why = "Block sizes must be powers of two!"; return 1; }
    if ((mode & BA_X_DROP) && x_drop < 0) { *why = "X-drop threshold amount must be nonnegative!"; return 1; }
    if ((mode & BA_LOCAL_START) && (mode & BA_FREE_QUERY_START_GAPS)) { *why = "Cannot set both LOCAL_START and FREE_QUERY_START_GAPS!"; return 1; }
    if ((mode & BA_X_DROP) && (mode & BA_FREE_QUERY_END_GAPS)) { *why = "Cannot set both X_DROP and FREE_QUERY_END_GAPS!"; return 1; }
    return 0;
}

constexpr size_t BA_MAX_BLOCK = 32768;   // the reference takes any power of two below 65535 (scan_block.rs:855)
static int pclass_of(size_t max_size) {   // index into {1,2,4,8,16} packed registers per lane; 5 = tiled (blocks above 2048 cells)
    if (max_size <= 128) return 0;
    if (max_size == 256) return 1;
    if (max_size == 512) return 2;
    if (max_size == 1024) return 3;
    if (max_size == 2048) return 4;
    if (max_size == 4096 || max_size == 8192 || max_size == 16384 || max_size == 32768) return BA_PCLASS_BIG;
    return -1;
}
static inline uint32_t lds_class_cells(int pc) { return pc == BA_PCLASS_BIG ? 128u : 128u << pc; }   // LDS layout class of a kernel class

// Build a batch from already-converted byte ranges. `get(p, which, &ptr, &len)` yields pair p's query (0) / reference (1).
// AAProfile -> device image (layout in ba_params.h). `P` positions, defaults (-128) beyond the profile's own length.
static void profile_image(const AAProfile* pr, uint32_t P, uint8_t* dst) {
    int8_t* pos_aa = (int8_t*)dst;
    int16_t* aa_pos = (int16_t*)(dst + (size_t)P * 32);
    int16_t* goC = aa_pos + (size_t)P * 32; int16_t* clC = goC + P; int16_t* goR = clC + P;
    const size_t have = std::min<size_t>(P, pr->curr_len);
    memset(pos_aa, 0x80, (size_t)P * 32);
    memcpy(pos_aa, pr->pos_aa.data(), have * 32);
    for (size_t c = 0; c < 32; c++)
        for (size_t i = 0; i < P; i++) aa_pos[c * P + i] = (int16_t)pos_aa[i * 32 + c];    // scores.rs:552-553 keeps both orders in sync
    for (size_t i = 0; i < P; i++) {
        goC[i] = i < have ? pr->gap_open_C[i] : (int16_t)-128;
        clC[i] = i < have ? pr->gap_close_C[i] : (int16_t)-128;
        goR[i] = i < have ? pr->gap_open_R[i] : (int16_t)-128;
    }
}
struct NoProfiles { const AAProfile* operator()(size_t) const { return nullptr; } };

constexpr size_t POOL_SLACK = 256;
// Seed-and-extend batches (ba_extend_batch_*): every pair's query / reference is a slice of the caller's bytes, which are on the device
// already (uploaded once, [host_base, host_base + bytes) at dev_base); k_pack_images cuts the images out of them, reversed and / or
// complemented as `flags` says (2 per pair, caller's order: query, reference; ba::IMG_*). seed_of names the seed a pair belongs to.
struct ExtImages {
    const uint8_t* host_base = nullptr; const uint8_t* dev_base = nullptr;
    const uint8_t* flags = nullptr;
    const uint32_t* seed_of = nullptr;
    float* pack_ms = nullptr;   // (optional) device time of the packer
    const char* what = "seed";  // what seed_of counts, for the message about a byte outside the alphabet (chain batches: "chain")
};
struct Packed {   // host-side packing of a set of pairs: padded images + the per-pair arrays the kernels read
    std::vector<uint64_t> qo, ro, cig_off;
    std::vector<uint32_t> ql, rl;
    std::vector<uint8_t> image;
    uint64_t total = 0, maxlen2 = 0, cig_total = 0;
    // Sequences that come out of one contiguous host buffer are not padded on the host: the raw bytes [raw, raw + raw_bytes)
    // go to the device as they are and k_pack_sequences builds the images there (raw_qo / raw_ro: offsets into raw).
    bool on_device = false;
    const uint8_t* raw = nullptr; uint64_t raw_bytes = 0; uint32_t pad = 0;
    std::vector<uint64_t> raw_qo, raw_ro;
    const ExtImages* ext = nullptr; std::vector<uint8_t> ext_flags;   // extension images (device order, 2 per pair)
    // Device order: entry s of every array above describes the caller's pair order[s] (empty = the caller's order). The
    // waves take pairs in device order, which is longest first (greedy longest-processing-time): no wave starts a long pair
    // when the rest of the batch is done. Lognormal protein lengths (22..8881, SURVEY 8d's config 4): +16 % score only,
    // +31 % with traceback against the caller's order (tools/lpt_experiment.py). Results are handed back in the caller's order.
    std::vector<uint32_t> order;
    size_t who(size_t s) const { return order.empty() ? s : order[s]; }
};
template <class GetSeq, class GetProfile, class Lap>
static int pack_pairs_in_order(int kind, Gaps gaps, size_t min_size, size_t max_size, uint32_t mode, size_t n, bool already_converted,
                               GetSeq get, GetProfile getp, Packed& P, Lap lap, const ExtImages* ext = nullptr) {
    const bool profile = kind == BA_KIND_PROFILE_;
    // ---- PaddedBytes images: [NULL] + bytes + NULL x (max_size + 16)
    const size_t pad = max_size + 16;
    std::vector<uint64_t>& qo = P.qo; std::vector<uint64_t>& ro = P.ro;
    qo.resize(n); ro.resize(n);
    std::vector<uint32_t>& ql = P.ql; std::vector<uint32_t>& rl = P.rl;
    ql.resize(n); rl.resize(n);
    uint64_t total = 0, maxlen2 = 0, cig_total = 0;
    std::vector<uint64_t>& cig_off = P.cig_off;
    cig_off.resize(n + 1);
    const uint8_t* lo = nullptr; const uint8_t* hi = nullptr; uint64_t sum_len = 0;   // extent of the caller's bytes
    auto span = [&](const uint8_t* ptr, size_t len) {
        if (!lo || ptr < lo) lo = ptr;
        if (!hi || ptr + len > hi) hi = ptr + len;
        sum_len += len;
    };
    for (size_t p = 0; p < n; p++) {
        const uint8_t* ptr; size_t len;
        get(p, 0, &ptr, &len);
        if (len > 0x3fffffffu) { fail("sequence too long"); return 1; }
        span(ptr, len);
        ql[p] = (uint32_t)len; qo[p] = total; total += (1 + len + pad + 3) & ~(size_t)3;   // images start 4-byte aligned
        if ((mode & BA_FREE_QUERY_END_GAPS) && !(min_size > len)) {   // scan_block.rs:860-862
            fail("pair %zu: Min block size must be larger than the query length for FREE_QUERY_END_GAPS!", P.who(p)); return 1;
        }
        if (profile) {
            const AAProfile* pr = getp(p);
            if (!pr) { fail("pair %zu: null profile", P.who(p)); return 1; }
            if (pr->gap_extend != gaps.extend) { fail("pair %zu: profile gap_extend %d differs from the batch's %d", P.who(p), pr->gap_extend, gaps.extend); return 1; }
            len = pr->str_len;
            if (len > 0x3fffffffu) { fail("profile too long"); return 1; }
            rl[p] = (uint32_t)len; ro[p] = total; total += ba::profile_image_bytes((uint32_t)len, (uint32_t)max_size);
        } else {
            get(p, 1, &ptr, &len);
            if (len > 0x3fffffffu) { fail("sequence too long"); return 1; }
            span(ptr, len);
            rl[p] = (uint32_t)len; ro[p] = total; total += (1 + len + pad + 3) & ~(size_t)3;
        }
        maxlen2 = std::max<uint64_t>(maxlen2, (uint64_t)ql[p] + rl[p] + 2);
        cig_off[p] = cig_total;
        cig_total += (uint64_t)ql[p] + rl[p] + 1;
    }
    cig_off[n] = cig_total;
    total += POOL_SLACK;   // behind the last image: the kernels read whole 128-byte rows of a block unpredicated (prefetch_seq)
    lap("offsets");
    P.total = total; P.maxlen2 = maxlen2; P.cig_total = cig_total; P.pad = (uint32_t)pad;
    if (ext) {   // extension images: always cut on the device, out of the caller's bytes uploaded once
        P.on_device = true; P.ext = ext; P.raw = ext->host_base;
        P.raw_qo.resize(n); P.raw_ro.resize(n); P.ext_flags.resize(2 * n);
        for (size_t p = 0; p < n; p++) {
            const uint8_t* ptr; size_t len;
            get(p, 0, &ptr, &len); P.raw_qo[p] = (uint64_t)(ptr - ext->host_base);
            get(p, 1, &ptr, &len); P.raw_ro[p] = (uint64_t)(ptr - ext->host_base);
            P.ext_flags[2 * p] = ext->flags[2 * P.who(p)]; P.ext_flags[2 * p + 1] = ext->flags[2 * P.who(p) + 1];
        }
        lap("extension image offsets");
        return 0;
    }
    // One dense host buffer (the pooled batch calls): ship it as it is, pad and convert on the device. Scattered or
    // overlapping sources (PaddedBytes handles, a reference shared by many pairs) and profile batches are packed here.
    if (!profile && !already_converted && n >= 256 && n < (1u << 30) && (uint64_t)(hi - lo) <= 2 * sum_len + 4096 && !dev_env("BA_HOST_PACK")) {
        P.on_device = true; P.raw = lo; P.raw_bytes = (uint64_t)(hi - lo);
        P.raw_qo.resize(n); P.raw_ro.resize(n);
        for (size_t p = 0; p < n; p++) {
            const uint8_t* ptr; size_t len;
            get(p, 0, &ptr, &len); P.raw_qo[p] = (uint64_t)(ptr - lo);
            get(p, 1, &ptr, &len); P.raw_ro[p] = (uint64_t)(ptr - lo);
        }
        lap("raw offsets");
        return 0;
    }
    std::vector<uint8_t>& image = P.image;
    image.assign(total, null_byte(kind));
    lap("image allocation + padding");
    {   // convert / copy the sequences into their padded images: independent per pair, spread over host threads
        unsigned nthreads = std::thread::hardware_concurrency();
        if (nthreads > 16) nthreads = 16;
        if (nthreads < 1 || n < 4096) nthreads = 1;
        std::vector<size_t> bad(nthreads, (size_t)-1);
        std::vector<uint8_t> bad_byte(nthreads, 0);
        auto work = [&](unsigned t) {
            for (size_t p = (size_t)n * t / nthreads; p < (size_t)n * (t + 1) / nthreads; p++) {
                if (profile) profile_image(getp(p), ba::profile_positions(rl[p], (uint32_t)max_size), image.data() + ro[p]);
                for (int w = 0; w < (profile ? 1 : 2); w++) {
                    const uint8_t* ptr; size_t len;
                    get(p, w, &ptr, &len);
                    uint8_t* dst = image.data() + (w ? ro[p] : qo[p]) + 1;
                    if (already_converted) memcpy(dst, ptr, len);
                    else for (size_t k = 0; k < len; k++) {
                        if (!convert_char(kind, ptr[k], dst + k)) { if (bad[t] == (size_t)-1) { bad[t] = p; bad_byte[t] = ptr[k]; } break; }
                    }
                }
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nthreads; t++) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
        for (unsigned t = 0; t < nthreads; t++)
            if (bad[t] != (size_t)-1) { fail("pair %zu: byte 0x%02x is outside the matrix alphabet", P.who(bad[t]), bad_byte[t]); return 1; }
    }
    lap("image fill");
    P.total = total; P.maxlen2 = maxlen2; P.cig_total = cig_total;
    return 0;
}

template <class GetSeq, class GetProfile, class Lap>
static int pack_pairs(int kind, Gaps gaps, size_t min_size, size_t max_size, uint32_t mode, size_t n, bool already_converted,
                      GetSeq get, GetProfile getp, Packed& P, Lap lap, const ExtImages* ext = nullptr) {
    std::vector<uint64_t> cost(n);   // cells to fill ~ (|q| + |r|) x block size
    for (size_t p = 0; p < n; p++) {
        const uint8_t* ptr; size_t len;
        get(p, 0, &ptr, &len); cost[p] = len;
        if (kind == BA_KIND_PROFILE_) { const AAProfile* pr = getp(p); cost[p] += pr ? pr->str_len : 0; }
        else { get(p, 1, &ptr, &len); cost[p] += len; }
    }
    P.order.resize(n);
    for (size_t p = 0; p < n; p++) P.order[p] = (uint32_t)p;
    std::stable_sort(P.order.begin(), P.order.end(), [&](uint32_t a, uint32_t c) { return cost[a] > cost[c]; });
    bool identity = true;
    for (size_t p = 0; p < n && identity; p++) identity = P.order[p] == p;
    if (identity || dev_env("BA_CALLER_ORDER")) P.order.clear();
    lap("longest-first order");
    const std::vector<uint32_t>& order = P.order;
    if (order.empty()) return pack_pairs_in_order(kind, gaps, min_size, max_size, mode, n, already_converted, get, getp, P, lap, ext);
    return pack_pairs_in_order(kind, gaps, min_size, max_size, mode, n, already_converted,
                               [&](size_t s, int w, const uint8_t** ptr, size_t* len) { get(order[s], w, ptr, len); },
                               [&](size_t s) { return getp(order[s]); }, P, lap, ext);
}

// Pair-slot batches: pair p's region of the trace arena holds its expected stack -- every step at the minimum block size, one
// grow sequence to the maximum, a few steps there -- times a margin (pct), never more than the reference's bound for the pair
// (Trace::new, scan_block.rs:1363-1366); its record list one entry per 4 residues. Pairs that outgrow their region report
// BA_ST_TRACE_OVERFLOW and are re-run by batch_wait. Returns the arena sizes in words / records.
static void pipe_regions(const BaBatch* b, const uint32_t* ql, const uint32_t* rl, size_t n, uint64_t pct, std::vector<uint64_t>& toff,
                         std::vector<uint64_t>& boff) {
    toff.resize(n + 1); boff.resize(n + 1);
    const uint64_t mx = b->max_size, mn = b->min_size;
    const uint64_t zm = (b->mode & BA_LOCAL_START) ? 2 : 1;   // (LOCAL_START: the zero masks, see batch_plan)
    // (k_small: the arena starts with the waves' sinks -- 64 lanes x 16 words each, where the slots without a step put their trace stores;
    // sized for any launch geometry: 4 workgroups of 8 waves per CU on up to 512 CUs)
    uint64_t t = b->small ? 512ull * 32 * 64 * 16 + 64 : 0, r = 0;
    t = (t + 15) & ~15ull;
    for (size_t p = 0; p < n; p++) {
        const uint64_t len2 = (uint64_t)ql[p] + rl[p] + 2;
        const uint64_t full = (mx / 16) * (len2 + 2 * mx) * 2 * zm + 64;
        const uint64_t want = (len2 * mn / 8 + mx * mx / 8 + 16 * mx) * zm * pct / 100 + 4096;
        toff[p] = t; t += (std::min(want, full) + 15) & ~15ull;
        boff[p] = r; r += len2 / 4 + 64;
    }
    toff[n] = t; boff[n] = r;
}
// Cut the arenas for the pairs (ql, rl). cap_words / cap_recs = 0: choose the margin by the free device memory (the caller
// allocates pipe_words / pipe_recs afterwards); otherwise the regions must fit the existing arenas. Returns 1 if they cannot.
// Device memory a batch may plan with: what is free, or -- while ba_sized_batch_create builds one batch per block range -- this batch's share of it
// (the ranges' batches are alive together and launched one after the other: each sized as if it were alone, the first ones took everything)
static thread_local uint64_t g_mem_cap = ~0ull;
static void mem_info(size_t* free_b, size_t* total_b) {
    *free_b = 0; *total_b = 0;
    (void)hipMemGetInfo(free_b, total_b);
    if ((uint64_t)*free_b > g_mem_cap) *free_b = (size_t)g_mem_cap;
}
static int pipe_cut(BaBatch* b, const uint32_t* ql, const uint32_t* rl, size_t n, uint64_t fixed_bytes, std::vector<uint64_t>& toff, std::vector<uint64_t>& boff) {
    size_t free_b = 0, total_b = 0;
    mem_info(&free_b, &total_b);
    uint64_t forced = 0;   // (development / test switch, as for the ring slots)
    if (const char* env = dev_env("BA_TRACE_MARGIN_PCT")) { int v = atoi(env); if (v > 0) forced = (uint64_t)v; }
    // (LOCAL_START: pairs that start in unrelated sequence sit at the maximum block size until the alignment is found -- 1 kbp pairs behind 100..300
    // unrelated bases, 50 k pairs: 2.2 % of them outgrew 175 % and were run again, 0.15 % outgrow 300 %)
    const bool local = b->mode & BA_LOCAL_START;
    for (uint64_t pct : {local ? 300ull : 175ull, local ? 175ull : 140ull, 110ull}) {
        if (forced) pct = forced;
        pipe_regions(b, ql, rl, n, pct, toff, boff);
        if (b->pipe_words) { if (toff[n] <= b->pipe_words && boff[n] <= b->pipe_recs) return 0; }
        else if (toff[n] * 4 + boff[n] * sizeof(BlockRec) + fixed_bytes + (1ull << 30) <= (uint64_t)free_b * 85 / 100) return 0;
    }
    return 1;
}

// ------------------------------------------------------------------ the kernel of a batch
// The one place that maps what batch_build chose to a kernel family. (A quad batch's own kernel is the per-pair one, which finishes the pairs k_quad
// hands over: b->grid and b->lds are that kernel's. k_quad itself is kernel_of(b, true).)
static ba::KernelFamily family_of(const BaBatch* b) {
    if (b->pclass == BA_PCLASS_BIG) return ba::FAM_TILED;
    if (b->multi) return b->geom == 2 ? ba::FAM_MULTI_G2 : (b->geom ? ba::FAM_MULTI_G3 : (b->multi_b == 512 ? ba::FAM_MULTI_512 : (b->multi_b == 256 ? ba::FAM_MULTI_256 : ba::FAM_MULTI)));
    return b->small ? ba::FAM_SMALL : ba::FAM_PAIR;
}
static const ba::KernelEntry* kernel_of(const BaBatch* b, bool quad = false) {
    const int family = quad ? ba::FAM_QUAD : family_of(b), pc = quad ? 0 : (int)b->pclass, special = quad ? 0 : special_of(b->mode);   // (k_quad: one per kind)
    const ba::KernelEntry* k = find_kernel(family, b->kind, pc, special);
    if (!k) fail("no kernel of family %d for kind %d, block class %d, %s modes", family, b->kind, pc, special ? "special" : "plain");
    return k;
}
// ... and what else depends on the family: LDS bytes per workgroup, bytes per wave in the `big` arena
static uint32_t kernel_lds_bytes(const BaBatch* b) {
    const uint32_t cells = lds_class_cells((int)b->pclass);   // (sized by the block class 128 << pc, as the kernels lay it out)
    switch (family_of(b)) {
    case ba::FAM_PAIR: case ba::FAM_TILED:   // + the traceback wave's windows (the special modes' walk records also hold zero-mask bits)
        return ba::lds_wg_bytes_h(b->kind, cells) + ((b->mode & BA_TRACE) ? (special_of(b->mode) ? ba::TB_LDS_BYTES_LOC : ba::TB_LDS_BYTES) : 0u);
    case ba::FAM_SMALL: return ba::sm_wg_bytes_h(b->kind, cells);
    default: return ba::mq_wg_bytes_h(b->kind, cells, b->wpw);   // (k_multi's traceback waves keep their records in their own wave's region: no extra space)
    }
}
static size_t kernel_wave_arena_bytes(const BaBatch* b) {
    switch (family_of(b)) {
    case ba::FAM_PAIR: return 0;
    case ba::FAM_TILED: return ba::big_wave_shorts(b->max_size) * sizeof(short);
    case ba::FAM_SMALL: return ba::SM_WAVE_BYTES;
    default: return ba::MQ_WAVE_BYTES;
    }
}
// The kernel of the entry for the batch's X_DROP bit, with / without traceback; bp's flags choose the form where the family has two.
static const void* kernel_fn(const BaBatch* b, const ba::KernelEntry* k, bool trace, int form) {
    const int xd = (b->mode & BA_X_DROP) != 0;
    if (trace && k->fn64[form][xd] && b->pool64()) return k->fn64[form][xd];   // (k_multi: the large-pool form is a kernel of its own)
    return k->fn[form][trace][xd];
}
static hipError_t kernel_lds_opt_in(const void* fn, unsigned lds) {   // more than the default dynamic-LDS limit: opt in (160 KB per CU on gfx950)
    return lds > 64 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}
static hipError_t kernel_launch(const BaBatch* b, const ba::KernelEntry* k, bool trace, unsigned grid, unsigned lds, hipStream_t s, const BatchParams* bp) {
    const void* fn = kernel_fn(b, k, trace, (k->fn[1][0][0] && !(bp->flags & ba::F_LOCAL)) ? 1 : 0);
    if (hipError_t e = kernel_lds_opt_in(fn, lds)) return e;
    void* args[] = {(void*)bp};
    return hipLaunchKernel(fn, dim3(grid), dim3(k->wpw * 64), args, lds, s);
}
static hipError_t kernel_occupancy(const BaBatch* b, const ba::KernelEntry* k, bool trace, unsigned lds, int* blocks_per_cu) {
    *blocks_per_cu = 0;
    for (int form = 0; form < 2 && k->fn[form][0][0]; form++) {   // (two forms, one launch geometry for both: the smaller)
        const void* fn = kernel_fn(b, k, trace, form);
        int v = 0;
        if (hipError_t e = kernel_lds_opt_in(fn, lds)) return e;
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, fn, (int)k->wpw * 64, lds)) return e;
        *blocks_per_cu = form ? std::min(*blocks_per_cu, v) : v;
    }
    return hipSuccess;
}
// Workgroups of k_quad: what fits, at least 1 and at most 32 waves per CU, on every CU of the current device.
static int quad_grid(const BaBatch* b, uint32_t* grid) {
    const ba::KernelEntry* k = kernel_of(b, true);
    if (!k) return 1;
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (kernel_occupancy(b, k, (b->mode & BA_TRACE) != 0, k->lds, &per_cu) != hipSuccess || hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail("occupancy query failed for the small-block kernel");
    per_cu = std::max(1, std::min(per_cu, 32 / (int)k->wpw));
    *grid = (uint32_t)(prop.multiProcessorCount * per_cu);
    return *grid ? 0 : fail("occupancy query failed for the small-block kernel");
}

// Launch geometry and scratch sizes of a batch whose inputs are known: workgroups, LDS, trace slot size, traceback waves,
// slots per wave, hand-off ring. fixed_bytes = device memory the batch needs besides its per-wave scratch.
static int batch_plan(BaBatch* b, size_t n, uint64_t fixed_bytes, uint64_t maxlen2, bool full_trace, uint64_t avg_len2 = ~0ull) {
    const int kind = b->kind; const uint32_t mode = b->mode; const int pc = (int)b->pclass; const size_t max_size = b->max_size;
    const bool trace = mode & BA_TRACE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, b->device) != hipSuccess) { fail("hipGetDeviceProperties failed"); return 1; }
    const ba::KernelEntry* k = kernel_of(b);
    if (!k) return 1;
    b->lds = kernel_lds_bytes(b);
    if (b->lds > 160 * 1024) { fail("block size %zu needs %u bytes of LDS per workgroup", max_size, b->lds); return 1; }
    int per_cu = 0;   // (more than 64 KB: opted in per kernel, kernel_lds_opt_in)
    if (kernel_occupancy(b, k, trace, b->lds, &per_cu) != hipSuccess || per_cu <= 0) {
        fail("occupancy query failed for kind %d class %d (lds %u)", kind, pc, b->lds); return 1;
    }
    if (per_cu * b->wpw > 32) per_cu = 32 / b->wpw;
    if (b->geom && per_cu > (int)b->geom) per_cu = (int)b->geom;   // (a score-only instantiation needs fewer registers than its geometry allows: still that many waves per SIMD)
    if (const char* env = dev_env("BA_WGS_PER_CU")) { int v = atoi(env); if (v > 0) per_cu = v; }
    uint64_t grid = (uint64_t)prop.multiProcessorCount * per_cu;
    // (k_multi, score-only batches, round 6: no more waves than the batch fills with four pairs each -- a wave that finds fewer goes through them one
    // at a time, solo. 10 kbp pairs, two waves per SIMD: 8 k pairs 16.4 -> 12.1 ms, 7 k 18.3 -> 16.1; three: 11 k 20.0 -> 18.2. With traceback the spare
    // waves are the ones that walk: 8 k 23.9 -> 25.2 ms, 11 k 27.9 -> 28.1 -- not cut.)
    const uint64_t per_wg = (uint64_t)b->wpw * (b->small ? ba::SM_SLOTS : ((b->multi && b->geom && !trace) ? 512u / b->multi_b : 1u));   // (the eight-wave workgroups: 16 k pairs 22.9 -> 24.2 ms, not cut)
    const uint64_t need = (n + per_wg - 1) / per_wg;
    if (grid > need) grid = need;
    if (const char* env = dev_env("BA_GRID")) { int v = atoi(env); if (v > 0 && (uint64_t)v < grid) grid = (uint64_t)v; }   // (development: fewer workgroups)
    // trace stack capacity per slot: same bound as Trace::new (scan_block.rs:1363-1366), in 32-bit words
    // (LOCAL_START keeps a zero-mask word behind every trace word: x2)
    const uint64_t zm = (mode & BA_LOCAL_START) ? 2 : 1;
    b->trace_full = trace ? (uint64_t)(max_size / 16) * (maxlen2 + 2 * max_size) * 2 * zm + 64 : 0;   // (+ 64 words of slack: unpredicated stores of the fast path)
    b->trace_stride = b->trace_full;
    // That bound assumes the block sits at its maximum size for the whole alignment (11.9 MB per 10 kbp pair at 1024, of
    // which config 3 uses 1.8 MB). Large batches get slots sized for the expected stack instead -- every step at the minimum
    // size, one full grow sequence to the maximum, a few steps there -- times a margin; the few pairs that outgrow
    // their slot report BA_ST_TRACE_OVERFLOW on the device and are re-run with full-size slots by batch_wait.
    b->adaptive = false;
    // (... and the batches of a sized batch's block ranges, which share the device memory: full-size slots of long pairs at large blocks -- 140 MB
    // each -- left a range's batch a few dozen resident waves)
    // (round 6: ... and batches of long pairs -- a full-size slot of a 32 kbp pair at 4096 cells is 140 MB, 2500 of them left room for 1816 resident waves)
    if (trace && !full_trace && !dev_env("BA_FULL_TRACE_SLOTS") && (n >= 4096 || (maxlen2 >= 20000 && n >= 256) || g_mem_cap != ~0ull || dev_env("BA_ADAPTIVE_TRACE"))) {
        const uint64_t est = (maxlen2 * b->min_size / 8 + (uint64_t)max_size * max_size / 8 + 16ull * max_size) * zm;
        // margin over the expected stack, in percent (development / test switch: BA_TRACE_MARGIN_PCT). LOCAL_START, short pairs: see pipe_cut (long
        // pairs: the flanks are a small part of the stack, and a slot of 3 x 2 x the plain size halves the number of resident waves)
        uint64_t pct = ((mode & BA_LOCAL_START) && maxlen2 <= 4096) ? 500 : 175;   // (round 6: 500 -- at 300 the bench's LOCAL_START line re-ran 33 of its 50 000 pairs in a second launch; these slots are ~1 MB)
        // (k_multi, round 5: nine smaller slots per wave instead of eight -- config 3, same box: 8 x 175 % 163.1 ms / 104.9 GB, 9 x 150 % 161.5 / 101.2,
        // 10 x 125 % 161.9 / 93.8, 9 x 125 % 161.6 / 84.4; its stacks reach 93 % of the expected size, and a pair that outgrows its slot is run again)
        if (b->multi && !(mode & BA_LOCAL_START)) pct = 125;
        if (const char* env = dev_env("BA_TRACE_MARGIN_PCT")) { int v = atoi(env); if (v > 0) pct = (uint64_t)v; }
        const uint64_t want = est * pct / 100 + 4096;
        if (want < b->trace_full) { b->trace_stride = (want + 15) & ~15ull; b->adaptive = true; }   // (16-word multiples: LOCAL_START stores word pairs)
    }
    b->blocks_stride = trace ? maxlen2 : 0;
    if (b->trace_stride >= (1ull << 30)) { fail("trace stack of %llu words per pair exceeds the 2^30 limit", (unsigned long long)b->trace_stride); return 1; }
    if (trace) {
        // very long pairs: a trace slot can be hundreds of MB, so fewer waves may be resident than the chip could hold --
        // shrink the launch until one slot per wave fits in device memory (a long pair keeps its wave busy for long anyway)
        size_t free_b = 0, total_b = 0;
        mem_info(&free_b, &total_b);
        const uint64_t per_slot = b->trace_stride * 4 + b->blocks_stride * sizeof(BlockRec);
        const uint64_t fixed = fixed_bytes + (1ull << 30);
        const uint64_t budget = free_b * 9 / 10 > fixed ? free_b * 9 / 10 - fixed : 0;
        const uint64_t max_waves = per_slot ? budget / per_slot : ~0ull;
        if (max_waves < b->wpw) { fail("device memory: one workgroup's trace slots need %llu MB, %llu MB are free", (unsigned long long)(per_slot * b->wpw >> 20), (unsigned long long)(budget >> 20)); return 1; }
        if (grid * b->wpw > max_waves) grid = max_waves / b->wpw;
    }
    if (b->small) grid = std::min<uint64_t>(grid, 512ull * 32 / b->wpw);   // (the trace arena's sink area holds 512 x 32 waves: pipe_regions)
    b->grid = (uint32_t)grid;
    b->cq_grid = 0;
    if (b->quad) {   // the per-pair kernel beside k_quad: one workgroup per CU, so that k_quad always finds room next to it
        b->cq_grid = (uint32_t)std::min<uint64_t>(grid, (uint64_t)prop.multiProcessorCount);
        if (const char* env = dev_env("BA_CQ_GRID")) { int v = atoi(env); if (v > 0) b->cq_grid = (uint32_t)std::min<uint64_t>(grid, (uint64_t)v); }
    }
    // TRACE batches big enough to keep them busy get dedicated traceback waves (ba_driver.hpp traceback_consumer)
    // and several trace slots per fill wave, so a wave can start its next pair while earlier ones are being walked.
    b->tb_stride = 0; b->slots_per_wave = 1;
    b->n_fill_waves = b->grid * b->wpw;
    // Short pairs: a walk is a few hundred dependent steps, cheaper done at once by the fill wave's lane 0 than handed to a
    // traceback lane (protein pairs of ~300 residues, block 32..256: 202 vs 99 GCUPS; 1 kbp DNA pairs already prefer the hand-off).
    const bool short_pairs = kind != BA_KIND_PROFILE_ && avg_len2 <= 1024 && !dev_env("BA_FORCE_TB");
    {   // several short pairs per work-counter atomic; long pairs one by one (a chunk of long pairs would lengthen the launch's ragged end)
        const uint64_t waves = grid * b->wpw;
        const uint64_t by_len = avg_len2 != ~0ull ? 16384 / (avg_len2 + 1) : 1, by_n = waves ? n / (waves * 8) : 1;
        b->work_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, std::min(by_len, by_n)));
        if (b->small) b->work_chunk = 4;   // (sixteen slots refill one by one; pairs come longest first: a long chunk would queue the longest pairs on one wave)
        // (round 5: eight once the batch gives every slot two pairs and more -- 200 k 1 kbp pairs 8.15 -> 8.05 ms, 400 k protein pairs 3.74 -> 3.66; 2: 8.34 / 4.12; 16: 8.17 / 3.72)
        if (b->small && n >= 2 * waves * ba::SM_SLOTS) b->work_chunk = 8;
        if (const char* env = dev_env("BA_WORK_CHUNK")) { int v = atoi(env); if (v > 0) b->work_chunk = (uint32_t)v; }   // (development)
    }
    // Few pairs: while the batch gives a resident wave no more than about two pairs, the wave walks each path itself with all its lanes
    // (walk_wave: ~0.2 - 0.35 us per cell) instead of handing it to a traceback lane (64 walks in lockstep: 0.55 - 0.9 us per cell, the
    // better use of the machine once every wave has pairs waiting) -- 10 kbp pairs, block 128..1024, same box: 256 pairs 22.7 -> 12.6 ms,
    // 2048: 25.3 -> 13.2, 4096 (one per wave): 26.3 -> 19.3, 8192: 35.8 -> 33.5, 12000: 40.3 -> 48.1 (kept on the lanes).
    // (one pair per wave at most: in every block class; two: measured for the classes with large LDS regions only)
    uint64_t few_x = lds_class_cells(pc) >= 512 ? 2u : 1u;
    if (const char* env = dev_env("BA_FEW_PAIRS_X")) { int v = atoi(env); if (v >= 0) few_x = (uint64_t)v; }   // (development)
    const bool few_pairs = !special_of(mode) && n <= few_x * (uint64_t)grid * b->wpw && !dev_env("BA_FORCE_TB");
    if (trace && (b->grid >= 32 || (dev_env("BA_FORCE_TB") && b->grid >= 2)) && !short_pairs && !few_pairs && !b->pipe && !dev_env("BA_INLINE_TRACEBACK")) {
        // one traceback wave per 4 workgroups = per 31 fill waves: at config 3 one per 5 ties and one per 6 is
        // 3.5 % slower, so 4 leaves a margin for workloads with more traceback per filled cell. (Workgroup b runs on XCD
        // b % 8, so the traceback waves sit on XCDs 0 and 4 only; measured against stride 3 / 5 -- all XCDs -- this makes
        // no difference now that a walk runs out of LDS.)
        // (the traceback work per filled cell grows as the block shrinks: with blocks below 128 cells one wave per 3
        // workgroups -- 1 kbp DNA, block 32..256: 360 GCUPS against 285 at one per 4)
        uint32_t stride = b->grid >= 32 ? (b->min_size >= 128 ? 4 : 3) : 2;
        // (k_multi fills faster -- four pairs per wave, eight cells per lane -- and its walks are what it waits for: one traceback wave
        // per 2 workgroups. Config 3, same box: per 4: 217 ms, per 3: 200.4, per 2: 198.9)
        if (b->multi && b->grid >= 32) stride = 2;
        // (round 6: the lanes' walk takes runs of diagonal moves at once -- ~45 % fewer instructions per rectangle crossed -- and one traceback wave per
        // 3 workgroups keeps up: 85 more fill waves. Same box, per 2 / 3 / 4 / 6: 100 k pairs 159.2 / 158.3 / 159.8 / 188.8 ms, 50 k 90.2 / 89.1 / 88.6 / 97.1,
        // 12.5 k 36.4 / 34.2 / 33.9 / 34.1. The special modes' walks are the round-5 ones: per 2 as before.)
        if (b->multi && b->grid >= 32 && !special_of(mode)) stride = 3;
        // (the four-wave workgroups of round 6's geometries: the same share of the waves. 12 k pairs at three waves per SIMD, one per 4 / 6 / 8 workgroups:
        // 33.3 / 29.0 / 30.3 ms; 8 k pairs at two: 3 / 4 / 6: 28.3 / 27.4 / 23.3)
        if (b->multi && b->geom && b->grid >= 32) stride = 6;
        if (const char* env = dev_env("BA_TB_STRIDE")) { int v = atoi(env); if (v > 0) stride = (uint32_t)v; }
        b->tb_stride = stride;
        b->n_fill_waves = b->grid * b->wpw - (b->grid + stride - 1) / stride;
        size_t free_b = 0, total_b = 0;
        mem_info(&free_b, &total_b);
        const uint64_t per_slot = b->trace_stride * 4 + b->blocks_stride * sizeof(BlockRec);
        const uint64_t fixed = fixed_bytes + (1ull << 30);
        uint32_t spw = 4;   // one being filled + three pending walks per fill wave, HBM permitting (188 GB at config 3; 3 slots: -1 %, 2: -17 %, 5: no gain)
        const uint32_t mslots = b->multi ? 512u / b->multi_b : 0u;   // k_multi: pairs a wave fills at once (four slots of 128 cells, or two of 256)
        if (b->multi) spw = mslots + 5;   // four pairs being filled + pending walks (round 4: 8 instead of 10 -- 105 instead of 131 GB at config 3 for -0.7 %; round 5: 9, smaller -- see the margin above; 7: 190 ms, 6: 208)
        if (const char* env = dev_env("BA_SLOTS_PER_WAVE")) { int v = atoi(env); if (v > 0) spw = (uint32_t)v; }
        while (spw > 1 && fixed + per_slot * spw * b->n_fill_waves > free_b * 9 / 10) spw--;
        if (b->multi && spw < mslots + 2) return fail("device memory: the multi-pair kernel needs two trace slots per wave beside its pairs'");   // (batch_build falls back to the per-pair kernel)
        b->slots_per_wave = spw;
        // The last hand-offs of the batch go to fill waves that have run out of pairs (one walking lane per wave, on
        // SIMDs with nothing else left to do): a walk alone is much shorter than one among 40 in lockstep, and the
        // batch ends one walk after its last fill. Half of the fill waves (measured at config 3 with 3968 of them: flat between
        // 1000 and 2500, 0.6 % slower at 3000, more below 500); fewer than all of them, so the fill waves can never all be
        // waiting for trace slots whose walks are reserved for helpers that do not exist yet.
        b->tb_reserve = b->n_fill_waves / 2;
        // (k_multi, round 5: the emptied waves' whole-wave walks take runs of diagonal moves at once -- one per fill wave; config 3, same box:
        // 164.7 -> 163.3 ms, twice as many: 169.0; 50 k pairs 92.1 -> 91.0, 25 k 55.4 -> 53.5; at 16 k pairs, four per wave, half stays better: 42.7 / 43.1)
        // (why all of them is safe here although the rule above says "fewer than all": a k_multi fill wave only waits when every one of its trace
        // slots is taken -- four by its live pairs, the other spw - 4 >= 2 by pending walks --, so if EVERY fill wave waited there would be at
        // least 2 n_fill_waves hand-offs pending, more than the n_fill_waves reserved ones: some of them are the dedicated lanes', which are
        // resident and walking; and a wave that waits long walks a pending hand-off itself, traceback_help_one. Enforced below: spw >= 6.)
        // (round 6, the cheaper lane walk: one per fill wave at every batch size -- 12.5 k pairs 34.2 -> 33.6 ms, 25 k 49.4 -> 49.2, 100 k 158.3 -> 157.9)
        // (round 11, the whole-wave walk's runs cross rectangles: one per fill wave stays best -- same box, BA_TB_RESERVE at 1x / 1.5x / 2x the fill
        // waves: 100 k pairs 131.7 / 132.5 / 134.3 ms, 25 k pairs 41.1 .. 41.7 / 42.2 / 43.0 ms; profiles/r11_walk_runs.md)
        if (b->multi && (n >= 5ull * b->n_fill_waves || !special_of(mode)) && spw >= mslots + 2) b->tb_reserve = b->n_fill_waves;
        // with fewer than three trace slots per wave a fill wave soon waits for the walk of its previous pair: leave
        // less of the batch to walkers that only exist once the first wave has run out of pairs
        if (spw < 3) b->tb_reserve = b->n_fill_waves / 4;
        if (const char* env = dev_env("BA_TB_RESERVE")) b->tb_reserve = (uint32_t)std::max(0, atoi(env));
        // (whatever the switches say: the reserved hand-offs stay below what the fill waves' spare slots can hold pending)
        if (b->multi) b->tb_reserve = std::min<uint32_t>(b->tb_reserve, b->n_fill_waves * (spw > mslots ? spw - mslots : 1) - 1);
    }
    // (round 4: a quarter of the fill waves instead of all of them -- since waves that run out of pairs take over other waves' slots at the
    // end of the batch, fewer pairs need to be kept out of the slots: config 3 178.9 -> 176.7 ms, 25 k pairs 60.5 -> 58.0 ms; 0: the same)
    b->mq_drain = b->multi ? ((dev_env("BA_NO_DONATE") || !trace || special_of(mode)) ? b->n_fill_waves : b->n_fill_waves / 4) : 0;
    if (const char* env = dev_env("BA_MQ_DRAIN")) b->mq_drain = (uint32_t)std::max(0, atoi(env));
    if (b->multi && b->slots_per_wave < 512u / b->multi_b) b->slots_per_wave = 512u / b->multi_b;   // (without the hand-off ring: one trace slot per slot of the wave)
    b->slots = b->n_fill_waves * b->slots_per_wave;
    if (b->pipe) b->slots = (uint32_t)n;   // (slot = pair: slot_info holds one entry per pair for k_walk)
    {
        const uint64_t lanes = b->tb_stride ? (uint64_t)((b->grid + b->tb_stride - 1) / b->tb_stride) * 64 + b->n_fill_waves : 0;   // + one helper lane per fill wave
        uint64_t need_q = std::max<uint64_t>(lanes, b->slots);
        uint32_t qs = 1;
        while (qs < need_q) qs <<= 1;
        b->tb_qsize = qs;
    }

    return 0;
}
static int batch_alloc_scratch(BaBatch* b) {
#define BA_ALLOC(buf, bytes) if (b->buf.alloc(bytes)) return 1
    BA_ALLOC(trace, b->pipe ? b->pipe_words * 4 : b->trace_stride * 4 * b->slots);
    BA_ALLOC(blocks, b->pipe ? b->pipe_recs * sizeof(BlockRec) : b->blocks_stride * sizeof(BlockRec) * b->slots);
    BA_ALLOC(ckpt, (size_t)(b->grid + b->cq_grid) * b->wpw * 8 * b->max_size * sizeof(short));
    BA_ALLOC(big, (size_t)b->grid * b->wpw * kernel_wave_arena_bytes(b));
    BA_ALLOC(tb_queue, (size_t)b->tb_qsize * 4); BA_ALLOC(tb_ctrl, 256); BA_ALLOC(prof, 2048); BA_ALLOC(params_dev, sizeof(BatchParams));
    BA_ALLOC(slot_free, (size_t)b->slots * 4); BA_ALLOC(slot_info, (size_t)b->slots * sizeof(ba::SlotInfo)); BA_ALLOC(counter, 128);
    if (b->multi) BA_ALLOC(donate, ((size_t)b->grid * b->wpw + 64) * 4);   // (+ two counters in their own cache lines)
#undef BA_ALLOC
    return 0;
}

// Sequence images into b->pool; the per-pair offset / length arrays must already be on the device.
static int upload_images(BaBatch* b, const Packed& P, size_t n) {
    if (!P.on_device) { HIP_TRY(hipMemcpy(b->pool.p, P.image.data(), P.total, hipMemcpyHostToDevice)); return 0; }
    if (P.ext) {   // extension images: the caller's bytes are on the device already
        DevBuf raw_q, raw_r, flags, err;
        if (raw_q.alloc(n * 8) || raw_r.alloc(n * 8) || flags.alloc(2 * n) || err.alloc(8)) return 1;
        HIP_TRY(hipMemcpy(raw_q.p, P.raw_qo.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw_r.p, P.raw_ro.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(flags.p, P.ext_flags.data(), 2 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(err.p, 0xff, 8));
        HIP_TRY(hipMemset((uint8_t*)b->pool.p + P.total - POOL_SLACK, null_byte(b->kind), POOL_SLACK));
        HIP_TRY(hipEventRecord(b->ev0, b->stream));
        HIP_TRY(ba_launch_pack_images(b->stream, seq_kind(b->kind), P.ext->dev_base, raw_q.as<uint64_t>(), raw_r.as<uint64_t>(), flags.as<uint8_t>(),
                                      b->q_off.as<uint64_t>(), b->q_len.as<uint32_t>(), b->r_off.as<uint64_t>(), b->r_len.as<uint32_t>(),
                                      b->pool.as<uint8_t>(), P.pad, (uint32_t)n, err.as<unsigned long long>()));
        HIP_TRY(hipEventRecord(b->ev1, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (P.ext->pack_ms) HIP_TRY(hipEventElapsedTime(P.ext->pack_ms, b->ev0, b->ev1));
        unsigned long long e = 0;
        HIP_TRY(hipMemcpy(&e, err.p, 8, hipMemcpyDeviceToHost));
        if (e != ~0ull) return fail("%s %u: byte 0x%02x is outside the matrix alphabet", P.ext->what, P.ext->seed_of[P.who((size_t)(e >> 8))], (unsigned)(e & 0xff));
        return 0;
    }
    DevBuf raw, raw_q, raw_r, err;
    if (raw.alloc(P.raw_bytes) || raw_q.alloc(n * 8) || raw_r.alloc(n * 8) || err.alloc(8)) return 1;
    HIP_TRY(hipMemcpy(raw.p, P.raw, P.raw_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(raw_q.p, P.raw_qo.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(raw_r.p, P.raw_ro.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0xff, 8));
    HIP_TRY(hipMemset((uint8_t*)b->pool.p + P.total - POOL_SLACK, null_byte(b->kind), POOL_SLACK));   // slack behind the last image
    HIP_TRY(ba_launch_pack_sequences(b->stream, seq_kind(b->kind), raw.as<uint8_t>(), raw_q.as<uint64_t>(), raw_r.as<uint64_t>(),
                                     b->q_off.as<uint64_t>(), b->q_len.as<uint32_t>(), b->r_off.as<uint64_t>(), b->r_len.as<uint32_t>(),
                                     b->pool.as<uint8_t>(), P.pad, (uint32_t)n, err.as<unsigned long long>()));
    HIP_TRY(hipStreamSynchronize(b->stream));
    unsigned long long e = 0;
    HIP_TRY(hipMemcpy(&e, err.p, 8, hipMemcpyDeviceToHost));
    if (e != ~0ull) return fail("pair %zu: byte 0x%02x is outside the matrix alphabet", P.who((size_t)(e >> 8)), (unsigned)(e & 0xff));
    return 0;
}

// Is every score that involves the padding byte negative? Then no cell of a padding row or column can exceed the cells and borders it is
// computed from, which is what lets the kernels skip the padding columns of an X-drop alignment's last block (ba_driver.hpp run(), DESIGN.md
// section 4). The reference's index masks decide which entries that byte reads: a NucMatrix is indexed [c & 7][a & 15] (scores.rs:157,179), so
// 'Z' shares its row with 'B', 'J' and 'R' and its column with 'J' -- the whole row and the whole column count; an AAMatrix is indexed
// [c - 'A'][a - 'A'] with the padding at 26. Byte matrices (padding equals padding: a match) and profiles never qualify.
static bool pad_negative(int kind, const void* matrix) {
    const int8_t* m = (const int8_t*)matrix;
    if (!m) return false;
    if (kind == BA_KIND_NUC) {
        const int row = 'Z' & 7, col = 'Z' & 15;
        for (int a = 0; a < 16; a++) if (m[row * 16 + a] >= 0) return false;
        for (int c = 0; c < 8; c++) if (m[c * 16 + col] >= 0) return false;
        return true;
    }
    if (kind == BA_KIND_AA) {
        for (int a = 0; a < 27; a++) if (m[26 * 32 + a] >= 0 || m[a * 32 + 26] >= 0) return false;
        return true;
    }
    return false;
}
static int upload_dev_of(BaBatch* b);
static void plan_walks(BaBatch* b, const std::vector<uint32_t>& ql, const std::vector<uint32_t>& rl);
static void plan_exclusive(BaBatch* b, const std::vector<uint32_t>& ql, const std::vector<uint32_t>& rl);
// `get(p, which, &ptr, &len)` yields pair p's query (0) / reference (1); for kind PROFILE the reference comes from
// `getp(p)` instead.
template <class GetSeq, class GetProfile = NoProfiles>
static BaBatch* batch_build(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, size_t n,
                            bool already_converted, GetSeq get, GetProfile getp = GetProfile(), const ExtImages* ext = nullptr) {
    if (ensure_device()) return nullptr;
    const bool verbose = dev_env("BA_SETUP_TIMING") != nullptr;   // development: where the batch set-up time goes
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!verbose) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "block_aligner_hip setup: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    if (kind < 0 || kind > 3) { fail("unknown matrix kind %d", kind); return nullptr; }
    const bool profile = kind == BA_KIND_PROFILE_;
    const size_t min_size = size.min < 16 ? 16 : size.min, max_size = size.max < 16 ? 16 : size.max;   // clamp to L (scan_block.rs:853-854)
    std::string why;
    // (open == extend, a linear gap cost: the block kernels, as the reference, need open < extend, the exact full-matrix calls do not. Such a
    // batch is built for ba_*_exact and ba_*_exact_cigars; a launch is refused with the reference's message. Not for extension batches.)
    if (check_align_params(profile, gaps, min_size, max_size, x_drop, mode, &why, !ext)) { fail("%s", why.c_str()); return nullptr; }
    if (min_size > max_size) { fail("min block size exceeds max block size"); return nullptr; }
    if (profile && (mode & BA_CIGAR_EQ)) { fail("=/X CIGARs need two sequences; a profile alignment has none to compare"); return nullptr; }
    if (kind == BA_KIND_BYTES && (mode & BA_X_DROP)) { /* allowed by the reference, documented as inaccurate (scores.rs:235-239) */ }
    int pc = pclass_of(max_size);
    if (pc < 0) { fail("max block size %zu not supported by the HIP backend (16..%zu)", max_size, (size_t)BA_MAX_BLOCK); return nullptr; }
    if (n == 0 || n > 0x7fffffffu) { fail("batch must hold between 1 and 2^31-1 pairs"); return nullptr; }
    // Round 6: block ranges that end above 2048 cells but start well below (percent_len 1 % .. 10 % of a 20 .. 40 kbp read: 256 / 512 .. 4096). The
    // row-tiled class keeps a pair's borders in global memory and has neither the eight-cells-per-lane rectangles nor the untraced end-game grows --
    // and such a pair's block rarely passes 2048 cells. The batch is launched in the 2048-cell class (LDS borders, every fast path) with its own maximum;
    // a pair whose block wants to grow past 2048 cells stops with ST_CLASS_OVERFLOW and batch_wait runs it again in the row-tiled class (batch_retry).
    // 2500 pairs of 32 kbp at 512..4096, none of which passes 2048 cells, same box: 192.9 -> 140.1 ms with traceback, 132.5 -> 81.8 score only
    // (tools/dev/big_probe.sh).
    bool opt_class = false;
    // (from 128 cells: the small-block pipelines are not in the bet. A batch that loses the bet -- more than an eighth of its pairs re-run -- is launched
    // in the row-tiled class from its next run on: batch_drop_class_bet.)
    if (pc == BA_PCLASS_BIG && min_size >= 128 && min_size <= 1024 && !dev_env("BA_NO_OPT_CLASS")) { pc = 4; opt_class = true; }

    std::unique_ptr<BaBatch> b(new BaBatch);
    b->device = g_device; b->kind = kind; b->mode = mode; b->n = (uint32_t)n;
    b->min_size = (uint32_t)min_size; b->max_size = (uint32_t)max_size; b->pclass = (uint32_t)pc; b->opt_class = opt_class;
    b->gap_open = gaps.open; b->gap_extend = gaps.extend; b->x_drop = x_drop;

    Packed P;
    if (pack_pairs(kind, gaps, min_size, max_size, mode, n, already_converted, get, getp, P, lap, ext)) return nullptr;
    std::vector<uint64_t>& qo = P.qo; std::vector<uint64_t>& ro = P.ro; std::vector<uint32_t>& ql = P.ql; std::vector<uint32_t>& rl = P.rl;
    std::vector<uint64_t>& cig_off = P.cig_off;
    const uint64_t total = P.total, maxlen2 = P.maxlen2, cig_total = P.cig_total;
    b->h_q_off = qo; b->h_r_off = ro; b->h_order = P.order;
    plan_walks(b.get(), ql, rl);
    b->cap_n = n; b->cap_pool = total; b->cap_cig = cig_total; b->cap_maxlen2 = maxlen2;
    b->pool_bytes = total;

    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { fail("hipStreamCreate failed"); return nullptr; }
    if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) { fail("hipEventCreate failed"); return nullptr; }

    const bool trace = mode & BA_TRACE;
    const size_t mat_bytes = kind == BA_KIND_AA ? 27 * 32 : (kind == BA_KIND_NUC ? 8 * 16 : (profile ? 0 : 2));
    // ---- launch geometry: one wave per workgroup, as many resident waves as LDS / registers allow
    uint64_t sum_len2 = 0;
    for (size_t p = 0; p < n; p++) sum_len2 += (uint64_t)ql[p] + rl[p];
    // Small blocks: a 32-cell block keeps 16 of a wave's 64 lanes busy, so batches that start at 32 cells begin in k_quad, four
    // pairs to a wave, and only the pairs that need more than plain shift steps go on to the per-pair kernel (see batch_launch).
    // Small batches are bound by their longest pair's chain of steps, which the hand-over only lengthens: the pipeline is taken
    // from the sizes where it wins (measured, GCUPS with / without: protein pairs 32k 371 / 405, 64k 745 / 527, 400k 1375 / 597;
    // PSSM 8k 108 / 105, 20k 211 / 162, 80k 458 / 172; 1 kbp DNA 200k 1347 / 606). BA_FORCE_QUAD / BA_NO_QUAD override.
    // (1 kbp DNA, round 3 -- the per-pair kernel walks with whole waves now: 2.5 k pairs 0.78 / 1.89 ms without / with traceback against
    // 1.34 / 2.96 through the pipeline, 4 k 0.82 / 1.96 against 1.40 / 3.07, 8 k 1.37 / 3.18 against 1.44 / 3.31, 10 k 3.59 against 3.33)
    const size_t quad_from = kind == BA_KIND_AA ? 65536u : 8192u;
    const bool trace_mode = mode & BA_TRACE;
    b->quad = !special_of(mode) && pc != BA_PCLASS_BIG && min_size == 32 && !dev_env("BA_NO_QUAD") && (dev_env("BA_FORCE_QUAD") || n >= quad_from);
    // Round 4: sequence kinds take k_small instead (ba_small.hpp) -- sixteen pairs per wave at 32 cells, eight cells per lane, and the grow /
    // shrink / X-drop end game of a pair by the same wave in solo mode: no queue, no launch beside. Block classes up to 1024 cells.
    // From the batch sizes at which sixteen pairs per wave still fill the machine (same-box sweeps, tools/dev/small_sweep.sh; GCUPS k_small /
    // round-3 pipeline / per-pair kernel): 1 kbp DNA X-drop 40 k pairs 941 / 963 / 580, 80 k 1356 / 1154 / 622; with traceback 40 k 512 / 580 /
    // 348, 80 k 791 / 742 / 393; protein pairs 30 k 388 / 303 / 369, 70 k 792 / 651 / 519; with traceback 70 k 258 / 283 / 210, 150 k 487 / 441 /
    // 216. Below them the round-3 rules apply.
    size_t small_from = kind == BA_KIND_AA ? (trace_mode ? 98304u : 32768u) : (trace_mode ? 57344u : 49152u);
    if (profile) small_from = 10000u;   // (round 5: 11 k PSSM pairs 131 against 128 GCUPS, 20 k 227 against 208, 80 k 641 against 459; below: the round-2 pipeline)
    // (round 5: LOCAL_START / FREE_QUERY_START_GAPS batches of the sequence kinds too -- k_small's special instantiations; FREE_QUERY_END_GAPS stays per pair)
    // Same-box sweep (tools/dev/local_sweep.py: 1 kbp DNA pairs behind 100..300 unrelated bases, X-drop 50, block 32..256; GCUPS k_small / per-pair
    // kernel), since the per-pair kernel's register path takes these modes' steps: LOCAL_START with traceback 50 k pairs 367 / 470, 150 k 629 / 614,
    // 300 k 714 / 643; without 150 k 1077 / 1183, 300 k 1222 / 1187. (Before: with traceback 150 k 529 / 478, without 250 k 1009 / 857; with the zero
    // mask at four words per trace word 150 k 440 / 327.) FREE_QUERY_START_GAPS on the same pairs stays behind the per-pair kernel (150 k pairs with
    // traceback 662 / 782, without 1034 / 1294): those batches take k_small only when forced.
    const bool small_mode = !special_of(mode) || (!profile && !(mode & BA_FREE_QUERY_END_GAPS));
    if (mode & BA_LOCAL_START) small_from = trace_mode ? 196608u : 262144u;
    if ((mode & BA_FREE_QUERY_START_GAPS) && !dev_env("BA_FORCE_SMALL")) small_from = ~(size_t)0;
    b->small = small_mode && pc <= 3 && min_size == ba::SM_B_HOST && !dev_env("BA_NO_SMALL") && (dev_env("BA_FORCE_SMALL") || (n >= small_from && !dev_env("BA_FORCE_QUAD")));
    if (b->small) b->quad = false;
    // Pair-slot batches: every pair's trace stack stays in its own region of the arenas until the fill is over, then k_walk
    // walks all paths with one pair per lane. The small-block pipeline needs this form with TRACE; profile batches without small
    // blocks take it in place of the hand-off ring (50..500 positions, 20k pairs: 143 -> 158 GCUPS, 80k: 172 -> 225). Short
    // sequence pairs do not: their walks are few hundred steps, cheapest done at once by the fill wave's lane 0 (protein pairs,
    // 8k..65k pairs: 3 .. 20 % slower with k_walk, whose latest wave ends one longest-path walk after the fill).
    std::vector<uint64_t> toff, boff;
    if (trace && (!special_of(mode) || b->small) && pc != BA_PCLASS_BIG && (b->quad || b->small || (profile && n >= 4096) || dev_env("BA_FORCE_PIPE"))) {
        const uint64_t fixed = total + cig_total * 4 + (uint64_t)n * (64 + sizeof(ba::PairCont) + 40);
        if (!dev_env("BA_NO_PIPE") && !pipe_cut(b.get(), ql.data(), rl.data(), n, fixed, toff, boff)) {
            b->pipe = true; b->pipe_words = toff[n] + toff[n] / 8; b->pipe_recs = boff[n] + boff[n] / 8;   // (headroom for ba_batch_reload)
        }
    }
    if (trace && !b->pipe) b->quad = b->small = false;   // with TRACE the pipeline needs every pair's trace stack resident until the end
    // Batches that start at 128 cells (the reference's nanopore set-up, examples/nanopore_bench.rs: 1 % .. 10 % of 10 kbp): four pairs
    // per wave while a pair's block is 128 cells (ba_multi.hpp), from the sizes at which every wave still finds four pairs.
    // (round 5: LOCAL_START / FREE_QUERY_START_GAPS batches too -- k_multi's special instantiations; FREE_QUERY_END_GAPS stays per pair)
    // Round 5 (tools/dev/multi_from.py, tools/dev/tail_knobs.sh; GCUPS k_multi / per-pair kernel, block 128..512, same box): the pairs must be long enough
    // -- a pair's first block and its end game are the solo driver's, whose traced instantiation spills (section 4): with traceback, 30 k pairs of
    // 1000 bases 1040 / 1105, 1500 bases 1181 / 1085, 2000 bases 1257 / 1075; 300..1500 bases with a 10..120-base indel each 415 / 1014 at 20 k
    // pairs, 667 / 1112 at 200 k (before this rule those batches took k_multi); score-only 1361 / 1808 at 20 k, 2109 / 1925 at 60 k. Long pairs from
    // 12 288 pairs on (config 3's pairs: 10 k 1005 / 975, 12.5 k 1107 / 1054, 14 k 1198 / 1119).
    const uint64_t avg_len2 = n ? sum_len2 / n : 0;
    // (round 6, the cheaper lane walk and one traceback wave per 3 workgroups: config 3's pairs 10 k 1068 / 1050, 12 k 1290 / 1071, 12.5 k 1342 / 1105 -> from 10 000 pairs)
    bool multi_fits = avg_len2 >= 3000 ? n >= 10000 : (!trace_mode && n >= 49152);
    // Round 6: batches that start at 256 cells -- what percent_len gives reads above 12.8 kbp (lib.rs:109-111, examples/nanopore_bench_global.rs:144-171) --
    // take k_multi with two slots of 256 cells per wave: DNA, block classes 512 .. 2048, the plain modes. From the sizes at which every wave finds its two pairs.
    b->multi_b = 128;
    bool wide = false;
    if (min_size == 256 && kind == BA_KIND_NUC && !special_of(mode) && max_size >= 512 && pc >= 2 && pc <= 4) {
        wide = true; b->multi_b = 256;
        // (round 6, later: a wave whose second slot stays empty goes on stepping with the first -- from 256 pairs: 600 pairs of 22 kbp at 256..4096 34.9 ms against the
        // per-pair kernel's 45.4, 1500 of 13 kbp at 256..2048 21.5 / 27.2. The figures of the earlier rule, from 2048 pairs:)
        multi_fits = avg_len2 >= 6000 && n >= 256;   // (13 kbp reads, 256..2048, with traceback, GCUPS two-pair slots / per-pair kernel, same box: 1.5 k pairs 353 / 410, 2.5 k 576 / 401, 4 k 990 / 552, 8 k 1155 / 603, 20 k 1555 / 654, 70 k 1873 / 720)
    }
    // Round 6: the launch geometry of k_multi by the batch size. The kernel is bound by vector issue, so a round of the batch -- every slot of every resident
    // wave filled once -- takes as long as a SIMD has waves; a batch of about one round is fastest on the geometry whose slots it just fills (four-wave
    // workgroups, two / three of them per CU = 32 / 48 slots per CU; at three waves per SIMD the traced driver also spills 171 registers instead of 344), while
    // batches of many rounds want four waves per SIMD (config 3's 100 k pairs: 157.5 ms against 168.7 at three). DNA, block classes 512 and 1024, plain modes.
    // 10 kbp pairs at 128..1024, ms at four / three / two waves per SIMD / per-pair kernel, same box (tools/dev/geom_sweep.sh, geom_sweep2.sh) --
    // with traceback: 6 k pairs 38.4 / 38.6 / 22.2 / 22.5, 8 k 40.9 / 27.0 / 23.3 / 28.6, 10 k 32.6 / 27.3 / 27.4 / 34.1, 12.5 k 33.3 / 30.4 / 32.0 / -, 14 k 34.7 / 32.2 / 34.4,
    // 16 k 35.4 / 34.2 / 36.7, 20 k 41.6 / 42.2, 25 k 48.7 / 53.1; score only: 8 k 18.2 / 22.5 / 16.4 / 15.0, 10 k 22.6 / 22.7 / 18.3 / 19.5, 12 k 27.5 / 18.1 / 23.7 / 22.1,
    // 14 k 24.1 / 19.1, 16 k 22.9 / 26.0, 20 k 26.6 / 30.0.
    b->geom = 0; b->wpw = ba::WAVES_PER_WG;
    const bool geom_ok = !wide && kind == BA_KIND_NUC && !special_of(mode) && (pc == 2 || pc == 3) && min_size == ba::MQ_B_HOST;   // (the instantiations that exist: ba_kernels.hip)
    if (geom_ok && avg_len2 >= 3000) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || cus <= 0) cus = 256;
        const uint64_t s2 = 32ull * (uint64_t)cus, s3 = 48ull * (uint64_t)cus;   // slots of the two geometries
        // (where the geometries change over, tools/dev/geom_edges.sh -- with traceback, two / three waves per SIMD: 8.4 k pairs 25.6 / 27.5 ms, 9 k 26.4 / 27.0, 9.5 k 27.1 / 27.1;
        // three / four: 16 k 34.0 / 35.4, 17.5 k 40.1 / 39.7, 19 k 40.9 / 40.2; two / per-pair kernel: 5.5 k 20.4 / 22.3, 5 k - / 19.2. Score only (with the
        // workgroups cut to the batch, batch_plan; geom_edges3.sh): two / per-pair 7 k 16.1 / 14.1, 7.6 k 12.0 / 15.0, 9 k 13.5 / 17.2; two / three 9.2 k 13.4 / 17.8,
        // 9.5 k 18.3 / 17.7, 10.5 k 19.1 / 17.9; three / four 15 k 20.5 / 22.8, 15.5 k 26.0 / 23.0 -- steps, not slopes: a wave whose slots cannot all be refilled
        // finishes its pairs one at a time)
        if (trace_mode) {
            b->geom = n <= s2 * 115 / 100 ? 2u : (n <= s3 * 136 / 100 ? 3u : 0u);
            multi_fits = n >= s2 * 65 / 100;
        } else {
            b->geom = n <= s2 * 113 / 100 ? 2u : (n <= s3 * 124 / 100 ? 3u : 0u);
            multi_fits = n >= s2 * 92 / 100;
        }
    }
    if (const char* env = dev_env("BA_MQ_GEOM")) { const int v = atoi(env); b->geom = (geom_ok && (v == 2 || v == 3)) ? (uint32_t)v : 0u; }   // (development / tests: 0 = the eight-wave workgroups)
    // ... and batches that start at 512 cells (percent_len 1 % of reads above 25.6 kbp): one slot of 512 cells per wave -- the same pair per wave as the per-pair
    // kernel, but its plain steps in the slots' loop (the state in registers, the driver's decisions in vector code) instead of the per-pair driver's shell.
    if (min_size == 512 && kind == BA_KIND_NUC && !special_of(mode) && max_size >= 1024 && pc >= 3 && pc <= 4) {
        wide = true; b->multi_b = 512;
        // (32 kbp pairs at 512..4096, one slot per wave / per-pair kernel, same box, ms with traceback (tools/dev/m512_ab.sh): 300 pairs 54.3 / 84.6, 1200 54.6 / 85.0,
        // 2500 84.2 / 136.9, 5000 117.1 / 212.0; score only 600 pairs 26.2 / 48.8, 2500 64.9 / 81.6 -- a pair's own chain of steps is a third shorter)
        multi_fits = avg_len2 >= 8000 && n >= 256;
    }
    b->multi = !profile && small_mode && pc != BA_PCLASS_BIG && (min_size == ba::MQ_B_HOST || wide) && !dev_env("BA_NO_MULTI") && (dev_env("BA_FORCE_MULTI") || multi_fits);
    if (!b->multi) { b->multi_b = 128; b->geom = 0; }
    if (b->geom) b->wpw = (uint32_t)ba::MQ_GEOM_WPW;
    if (b->multi && batch_plan(b.get(), n, total + cig_total * 4 + (uint64_t)n * 64, maxlen2, false, sum_len2 / n)) { b->multi = false; b->geom = 0; b->wpw = ba::WAVES_PER_WG; }
    if (b->small && batch_plan(b.get(), n, total + cig_total * 4 + (uint64_t)n * 64, maxlen2, false, sum_len2 / n)) b->small = false;   // (e.g. LDS: falls back to the per-pair kernel)
    if (!b->multi && !b->small)
    if (batch_plan(b.get(), n, total + cig_total * 4 + (uint64_t)n * 64, maxlen2, false, sum_len2 / n)) return nullptr;
    if (b->pipe) b->adaptive = true;
    b->plan_fixed = total + cig_total * 4 + (uint64_t)n * 64; b->plan_maxlen2 = maxlen2; b->plan_avg = sum_len2 / n;
    plan_exclusive(b.get(), ql, rl);
    b->cig_total = trace ? cig_total : 0;

    lap("launch geometry");
#define BA_ALLOC(buf, bytes) if (b->buf.alloc(bytes)) return nullptr
    BA_ALLOC(pool, total); BA_ALLOC(q_off, n * 8); BA_ALLOC(q_len, n * 4); BA_ALLOC(r_off, n * 8); BA_ALLOC(r_len, n * 4);
    BA_ALLOC(matrix, 1024);
    BA_ALLOC(score, n * 4); BA_ALLOC(qidx, n * 4); BA_ALLOC(ridx, n * 4); BA_ALLOC(cig_len, n * 4); BA_ALLOC(cells, n * 8);
    BA_ALLOC(status, n * 4); BA_ALLOC(nblocks, n * 4); BA_ALLOC(pair_slot, n * 4); BA_ALLOC(trace_words, n * 4);
    BA_ALLOC(cig_off, (n + 1) * 8);
    BA_ALLOC(cig_ops, b->cig_total * 4);
#undef BA_ALLOC
    if (batch_alloc_scratch(b.get())) return nullptr;
    if (b->quad && (b->contA.alloc(n * sizeof(ba::PairCont)) || b->cont_n.alloc(n * 4))) return nullptr;
    if (b->pipe && (b->trace_off.alloc((n + 1) * 8) || b->blocks_off.alloc((n + 1) * 8))) return nullptr;
    if (b->quad) {
        if (b->cq_queue.alloc(n * 4) || b->cq_ctrl.alloc(256)) return nullptr;
        if (quad_grid(b.get(), &b->quad_grid)) return nullptr;
    }
    if ((b->quad || b->small) && (hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking) != hipSuccess ||
                               hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming) != hipSuccess)) {
        fail("hipStreamCreate / hipEventCreate failed"); return nullptr;
    }
    lap("device allocation");
#define BA_H2D(buf, src, bytes) if (hipMemcpy(b->buf.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { fail("hipMemcpy H2D failed"); return nullptr; }
    BA_H2D(q_off, qo.data(), n * 8); BA_H2D(q_len, ql.data(), n * 4);
    BA_H2D(r_off, ro.data(), n * 8); BA_H2D(r_len, rl.data(), n * 4); BA_H2D(cig_off, cig_off.data(), (n + 1) * 8);
    if (b->pipe) { BA_H2D(trace_off, toff.data(), (n + 1) * 8); BA_H2D(blocks_off, boff.data(), (n + 1) * 8); }
    if (upload_images(b.get(), P, n)) return nullptr;
    {
        int8_t tmp[1024] = {0};
        if (kind == BA_KIND_BYTES) { const ByteMatrix* bm = (const ByteMatrix*)matrix; tmp[0] = bm->match_score; tmp[1] = bm->mismatch_score; }
        else if (mat_bytes) memcpy(tmp, matrix, mat_bytes);
        BA_H2D(matrix, tmp, 1024);
        b->pad_negative = pad_negative(kind, matrix);
    }
#undef BA_H2D
    lap("host-to-device copies");
    if (hipMemset(b->cig_len.p, 0, n * 4) != hipSuccess || hipMemset(b->status.p, 0, n * 4) != hipSuccess) { fail("hipMemset failed"); return nullptr; }
    if (upload_dev_of(b.get())) return nullptr;
    return b.release();
}


// device copy of the caller-order -> device-order map (for the gather of CIGAR runs in the caller's order, ba_batch_compact_cigars)
static int upload_dev_of(BaBatch* b) {
    if (!(b->mode & BA_TRACE) || b->h_order.empty()) return 0;
    std::vector<uint32_t> dev_of(b->n);
    for (uint32_t s = 0; s < b->n; s++) dev_of[b->h_order[s]] = s;
    if (!b->dev_of.p && b->dev_of.alloc((size_t)b->cap_n * 4)) return 1;
    HIP_TRY(hipMemcpy(b->dev_of.p, dev_of.data(), (size_t)b->n * 4, hipMemcpyHostToDevice));
    return 0;
}

// Replace the pairs of an existing batch (same matrix, gaps, block range and modes); the device buffers -- above all the
// trace arena, whose allocation dominates the set-up time -- are reused, so the new set must fit what they were sized for.
template <class GetSeq, class GetProfile = NoProfiles>
static int batch_reload(BaBatch* b, size_t n, bool already_converted, GetSeq get, GetProfile getp = GetProfile(), const ExtImages* ext = nullptr) {
    if (!b) return fail("null batch");
    if (b->in_flight) return fail("reload: the batch has a launch in flight (ba_batch_wait first)");
    if (n == 0 || n > b->cap_n) return fail("reload: %zu pairs exceed the batch's capacity of %llu", n, (unsigned long long)b->cap_n);
    HIP_TRY(hipSetDevice(b->device));
    Packed P;
    if (pack_pairs(b->kind, Gaps{(int8_t)b->gap_open, (int8_t)b->gap_extend}, b->min_size, b->max_size, b->mode, n, already_converted, get, getp, P, [](const char*) {}, ext)) return 1;
    if (P.total > b->cap_pool) return fail("reload: %llu sequence bytes exceed the batch's capacity of %llu", (unsigned long long)P.total, (unsigned long long)b->cap_pool);
    if (P.maxlen2 > b->cap_maxlen2) return fail("reload: a pair is longer (%llu) than the longest pair the batch was created with (%llu)", (unsigned long long)P.maxlen2 - 2, (unsigned long long)b->cap_maxlen2 - 2);
    if ((b->mode & BA_TRACE) && P.cig_total > b->cap_cig) return fail("reload: CIGAR capacity exceeded");
    std::vector<uint64_t> toff, boff;
    if (b->pipe && pipe_cut(b, P.ql.data(), P.rl.data(), n, 0, toff, boff)) return fail("reload: the new pairs' trace regions exceed the batch's trace arena");
    // from here on the device arrays change: a failure leaves no pairs loaded (a later launch says so) instead of a mix
    b->n = 0; b->ran = false; b->loads++;
    HIP_TRY(hipMemcpy(b->q_off.p, P.qo.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->q_len.p, P.ql.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->r_off.p, P.ro.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->r_len.p, P.rl.data(), n * 4, hipMemcpyHostToDevice));
    if (upload_images(b, P, n)) return 1;
    HIP_TRY(hipMemcpy(b->cig_off.p, P.cig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    if (b->pipe) {
        HIP_TRY(hipMemcpy(b->trace_off.p, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->blocks_off.p, boff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemset(b->cig_len.p, 0, n * 4));
    HIP_TRY(hipMemset(b->status.p, 0, n * 4));
    b->n = (uint32_t)n; b->h_q_off = P.qo; b->h_r_off = P.ro; b->h_order = P.order; b->pool_bytes = P.total;
    plan_walks(b, P.ql, P.rl);
    plan_exclusive(b, P.ql, P.rl);
    b->cig_total = (b->mode & BA_TRACE) ? P.cig_total : 0;
    b->ran = false;
    return upload_dev_of(b);
}

// Enqueue one pass over the batch on its stream and return; batch_wait collects it. (Two batches on two streams
// overlap; with ba_batch_reload the host packs the next set while the device aligns the current one.)
// k_walk ends with its longest walk. A lane walks at ~0.55 us per cell, a whole wave on one path (walk_wave) several times faster but one
// path at a time and in scalar code (one scalar unit per CU: a few such walks per CU at most): the leading pairs of the batch order with at
// least 1 / BA_WALK_WAVE_FRAC of the longest pair's |q| + |r| -- at most BA_WALK_WAVE_MAX of them -- go one to a wave, the others one to a
// lane beside them, and the launch's makespan becomes the longest path at the wave's pace.
static void plan_walks(BaBatch* b, const std::vector<uint32_t>& ql, const std::vector<uint32_t>& rl) {
    uint32_t frac = 3, kmax = 1024;
    if (const char* e = dev_env("BA_WALK_WAVE_FRAC")) frac = (uint32_t)std::max(1, atoi(e));
    if (const char* e = dev_env("BA_WALK_WAVE_MAX")) kmax = (uint32_t)std::max(0, atoi(e));
    const size_t n = ql.size();
    uint32_t longest = 0;
    for (size_t p = 0; p < n; p++) longest = std::max(longest, ql[p] + rl[p]);
    const uint32_t from = std::max(longest / frac, 512u);
    // The walkers take the leading walk_wave_n pairs of the batch order. That order is longest first only when pack_pairs sorted it (it keeps
    // the caller's order when that is already sorted -- or when told to): then count the leading run; otherwise no pair is singled out rather
    // than an arbitrary prefix (round-3 advisor finding: an unsorted order stopped the prefix test at its first short pair).
    bool sorted = true;
    for (size_t p = 1; p < n && sorted; p++) sorted = (uint64_t)ql[p] + rl[p] <= (uint64_t)ql[p - 1] + rl[p - 1] + 64;   // (cost order: ties and near-ties in any order)
    size_t cnt = 0;
    if (sorted) while (cnt < n && cnt < kmax && ql[cnt] + rl[cnt] >= from) cnt++;
    // equal-length batches (every pair qualifies): whole-wave walks are for a FEW long paths beside many lane walks, not for a prefix of a
    // uniform batch
    if (cnt == std::min<size_t>(n, kmax) && n > kmax) cnt = 0;
    b->walk_wave_n = (uint32_t)cnt;
}
// k_small: sixteen pairs to a wave make every pair sixteen times as long in flight (and a neighbour's solo episode stops a slot), so a pair
// many times the average length would end the launch alone. The leading pairs of the batch order (longest first) whose own chain of steps
// in a slot would take more than about half of what the whole batch takes -- |q| + |r| above half the batch's residues per slot -- run one
// to a wave instead, on all lanes, before the wave starts its slots; at most one for every second wave.
static void plan_exclusive(BaBatch* b, const std::vector<uint32_t>& ql, const std::vector<uint32_t>& rl) {
    b->sm_excl_n = 0;
    if (!b->small || dev_env("BA_NO_EXCL")) return;
    const size_t n = ql.size();
    uint64_t total = 0;
    for (size_t p = 0; p < n; p++) total += (uint64_t)ql[p] + rl[p];
    const uint64_t slots = (uint64_t)b->grid * ba::WAVES_PER_WG * ba::SM_SLOTS;
    uint64_t thr = std::max<uint64_t>(total / std::max<uint64_t>(slots, 1) / 2, 1024);
    // ... and many times the batch's average length: a batch of equal pairs has none. (Score only: six times (~4000 for the protein set) -- same box, threshold
    // 2400 / 3600 / 4800 / 6000: 3.86 / 3.75 / 3.71 / 4.08 ms; with traceback the pairs' walks are part of the chain: 9.68 / 9.95 / - / 10.06 ms)
    thr = std::max<uint64_t>(thr, ((b->mode & BA_TRACE) ? 4 : 6) * (total / std::max<size_t>(n, 1)));
    // (no "the run did not end inside the cap" rule as in plan_walks: the protein set's 2048 longest of 400 k pairs fill the cap and are exactly the pairs
    // meant -- with that rule none ran alone and the launch took 8.05 instead of 3.8 ms)
    if (const char* e = dev_env("BA_EXCL_LEN2")) thr = (uint64_t)std::max(0, atoi(e));
    const size_t cap = (size_t)b->grid * ba::WAVES_PER_WG / 2;
    // (as in plan_walks: the leading pairs are the longest only when the device order is sorted -- it is not under BA_CALLER_ORDER --; an unsorted order
    // singles out no pair rather than an arbitrary prefix: round-5 advisor finding)
    bool sorted = true;
    for (size_t p = 1; p < n && sorted; p++) sorted = (uint64_t)ql[p] + rl[p] <= (uint64_t)ql[p - 1] + rl[p - 1] + 64;
    size_t cnt = 0;
    if (sorted) while (cnt < n && cnt < cap && (uint64_t)ql[cnt] + rl[cnt] > thr) cnt++;   // (device order: longest first)
    b->sm_excl_n = (uint32_t)cnt;
    // k_walk behind the fill: those pairs are walked by their own waves, so the paths it walks one to a wave (plan_walks: the leading pairs of the
    // batch order) are counted from the first pair that is NOT among them -- round 5: until then every pair k_walk saw went to a lane, and the launch
    // was as long as one lane's walk of the longest of them (400 k protein pairs: 2.08 ms for paths of up to ~2400 cells)
    if ((b->mode & BA_TRACE) && cnt && !special_of(b->mode) && !dev_env("BA_NO_WALK_AFTER_EXCL")) {
        const uint64_t first = (uint64_t)ql[cnt < n ? cnt : n - 1] + rl[cnt < n ? cnt : n - 1];
        const uint64_t from = std::max<uint64_t>(first / 3, 512);
        size_t w = cnt;
        while (w < n && w - cnt < 1024 && (uint64_t)ql[w] + rl[w] >= from) w++;
        b->walk_wave_n = (uint32_t)w;
    }
    // TRACE: the longest of them -- at least half the longest pair's length, at most one wave in thirty-two -- get a launch of their own
    // beside the main one (batch_launch): their fill + walk is a serial chain that outlasts the rest of the batch (400 k protein pairs with
    // traceback: the 8881-residue pair alone takes 8.6 ms, everything else 6 ms), and the walks of all other pairs need not wait for it
    size_t side = 0;
    // (development switch only: the two launches ran beside each other in one batch object and one after the other in the next -- 9.0 against
    // 15.3 ms for 400 k protein pairs with traceback, 10.8 without the second launch)
    if (dev_env("BA_EXCL_SIDE") && ((b->mode & BA_TRACE) || dev_env("BA_EXCL_SIDE_ALL")) && cnt) {
        const uint64_t longest = (uint64_t)ql[0] + rl[0];
        const size_t side_cap = std::max<size_t>(4, (size_t)b->grid / 8);   // (a workgroup of the side launch runs four pairs: at most one workgroup in 32)
        while (side < cnt && side < side_cap && ((uint64_t)ql[side] + rl[side]) * 2 >= longest) side++;
        if (b->grid < 16) side = 0;
    }
    b->sm_side_n = (uint32_t)side;
}
static uint32_t walk_grid(const BaBatch* b) {   // workgroups of k_walk (4 waves x 64 walking lanes each)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, b->device) != hipSuccess) return 1;
    uint32_t per_cu = 8;
    if (const char* env = dev_env("BA_WALK_WGS_PER_CU")) { int v = atoi(env); if (v > 0) per_cu = (uint32_t)v; }
    return std::min((b->n + 255u) / 256u + (b->walk_wave_n + 3u) / 4u, (uint32_t)prop.multiProcessorCount * per_cu);
}
// A batch launched in the 2048-cell class on the bet that few of its pairs grow past it (opt_class) whose last run lost the bet: plan and allocate it
// again as what its block range says -- the row-tiled class, per-pair kernel.
static int batch_drop_class_bet(BaBatch* b) {
    b->opt_class = false; b->bet_lost = false;
    b->pclass = (uint32_t)BA_PCLASS_BIG; b->multi = false; b->multi_b = 128; b->geom = 0; b->wpw = ba::WAVES_PER_WG;
    if (batch_plan(b, b->n, b->plan_fixed, b->plan_maxlen2, false, b->plan_avg)) return 1;
    return batch_alloc_scratch(b);
}
static int batch_launch(BaBatch* b) {
    if (b->in_flight) return fail("the batch already has a launch in flight (ba_batch_wait first)");
    // the buffers are about to be written again: what the last run left is no result from here on, whether this launch gets onto the stream,
    // times out or fails (ran is set again at the end of a successful batch_wait only)
    b->ran = false;
    b->compacted = false;
    if (b->n == 0) return fail("the batch holds no pairs (its last reload failed)");
    if (!b->handle_mode && b->kind != BA_KIND_PROFILE_ && b->gap_open == b->gap_extend)
        return fail("Gap open must cost more than gap extend! (a batch with open == extend serves the exact calls only)");
    HIP_TRY(hipSetDevice(b->device));
    if (b->bet_lost && batch_drop_class_bet(b)) return 1;
    if (!b->handle_mode) {   // (a handle's work counter arrives zeroed with its upload; it has no hand-off structures)
        HIP_TRY(hipMemsetAsync(b->counter.p, 0, 128, b->stream));
        HIP_TRY(hipMemsetAsync(b->tb_ctrl.p, 0, 256, b->stream));
        HIP_TRY(hipMemsetAsync(b->prof.p, 0, 2048, b->stream));
        HIP_TRY(hipMemsetAsync(b->tb_queue.p, 0, (size_t)b->tb_qsize * 4, b->stream));
        HIP_TRY(hipMemsetAsync(b->slot_free.p, 1, (size_t)b->slots * 4, b->stream));   // any non-zero value = free
        if (b->multi && b->donate.p) HIP_TRY(hipMemsetAsync(b->donate.p, 0, ((size_t)b->grid * b->wpw + 64) * 4, b->stream));
    }
    const BatchParams bp = b->params();
    HIP_TRY(hipEventRecord(b->ev0, b->stream));
    if (b->ev_l0) HIP_TRY(hipEventRecord(b->ev_l0, b->stream));   // (a re-run sub-batch: batch_retry re-uses ev0 for the merge)
    const ba::KernelEntry* k = kernel_of(b);
    const bool tr = b->mode & BA_TRACE, xd = b->mode & BA_X_DROP;
    if (!k) return 1;
    if (b->quad && b->n <= b->cap_n) {
        // k_quad starts every pair -- its first block and plain shift steps, four pairs per wave -- and finishes the global
        // alignments that never need more. A pair that does (a grow, X-drop termination, fewer than 32 residues) goes through a
        // queue to the per-pair kernel: one small launch of it runs beside k_quad on a second stream (the longest pairs come
        // first and leave early: their remaining steps are a long serial chain best started at once), a full-size one after it.
        // TRACE (a pair-slot batch): k_quad only stacks trace words; the paths of the pairs it finished are walked by k_walk, one
        // pair per lane, the per-pair kernel walks its own pairs' paths at once.
        const ba::KernelEntry* kq = kernel_of(b, true);
        if (!kq) return 1;
        uint32_t* flagA = b->cont_n.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(flagA, 0, (size_t)b->n * 4, b->stream));
        HIP_TRY(hipMemsetAsync(b->cq_queue.p, 0, (size_t)b->n * 4, b->stream));
        HIP_TRY(hipMemsetAsync(b->cq_ctrl.p, 0, 256, b->stream));
        HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
        BatchParams pq = bp; pq.cont_out = b->contA.as<ba::PairCont>(); pq.cont_out_flag = flagA;
        pq.cq_queue = b->cq_queue.as<uint32_t>(); pq.cq_ctrl = b->cq_ctrl.as<uint32_t>(); pq.cq_producers = b->quad_grid * ba::WAVES_PER_WG;
        pq.work_chunk = 4;   // (one position per slot: pairs come longest first, and a long chunk would queue the longest pairs on one wave)
        HIP_TRY(kernel_launch(b, kq, tr, b->quad_grid, kq->lds, b->stream, &pq));
        // (the pairs that reach the per-pair kernel -- with X-drop all of them, since termination is not a plain shift step: their
        // paths go to a second k_walk; without, only the pairs that grow: lane 0 walks each at once, nothing is left for the end)
        const bool walk2 = tr && bp.cig_ops && xd;
        pq.inline_len2 = walk2 ? ~0u : 0u;
        BatchParams pc = pq; pc.cont_mode = 2; pc.cont_in = b->contA.as<ba::PairCont>(); pc.cont_in_flag = flagA; pc.cont_out = nullptr; pc.cont_out_flag = nullptr;
        // Beside k_quad -- global alignments only: there the pairs that leave are the ones that grow, few and each a long serial
        // chain (protein pairs, 400k: 905 -> 1350 GCUPS; PSSM 80k: 349 -> 432); with X-drop every pair leaves and the per-pair
        // kernel has a full machine's worth of work after k_quad anyway (1 kbp DNA: 1320 -> 1226 with the side launch).
        // (launched after k_quad: a kernel that only waits must never be the one that holds the device)
        const bool beside = (!xd || dev_env("BA_CQ_BESIDE")) && !dev_env("BA_CQ_AFTER");
        if (beside) {
            BatchParams pa = pc; pa.ckpt_wave0 = b->grid * ba::WAVES_PER_WG; pa.cq_side = 1;
            HIP_TRY(hipStreamWaitEvent(b->stream2, b->ev_fork, 0));
            HIP_TRY(kernel_launch(b, k, tr, b->cq_grid, b->lds, b->stream2, &pa));
            HIP_TRY(hipEventRecord(b->ev_join, b->stream2));
        }
        if (tr && bp.cig_ops) {
            BatchParams w1 = bp; w1.cont_mode = 1; w1.cont_in_flag = flagA; w1.work_counter = b->counter.as<uint32_t>() + 8;   // (its own counter, zeroed above)
            HIP_TRY(ba_launch_walk(b->stream, &w1, walk_grid(b)));
        }
        HIP_TRY(kernel_launch(b, k, tr, b->grid, b->lds, b->stream, &pc));
        if (beside) HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_join, 0));
        if (walk2) {
            BatchParams w2 = bp; w2.cont_mode = 2; w2.cont_in_flag = flagA; w2.work_counter = b->counter.as<uint32_t>() + 12;
            HIP_TRY(ba_launch_walk(b->stream, &w2, walk_grid(b)));
        }
    } else if (b->small) {
        // k_small takes every pair from start to end (slots at 32 cells, everything else by the same wave in solo mode); TRACE: a pair-slot
        // batch -- the fill only stacks, k_walk (its form for slot rectangles) walks all paths afterwards
        // (the pairs run one to a wave at the start of the launch -- the batch's longest -- walk their paths at once, with the whole wave:
        // the longest walk of the batch overlaps with the fill instead of ending the launch)
        BatchParams p1 = bp; p1.inline_len2 = ~0u;
        const uint32_t side_n = (b->stream2 && !special_of(b->mode) && (bp.cig_ops || !(b->mode & BA_TRACE)) && b->sm_side_n && b->sm_side_n <= b->sm_excl_n) ? b->sm_side_n : 0u;
        uint32_t grid_main = b->grid;
        if (side_n) {
            // The longest pairs' launch: one wave per pair, workgroups taken off the main launch (together they fill the device as one
            // launch would); its waves use the tail of the wave-indexed scratch (arena, checkpoints). k_walk_l2 skips these pairs -- their
            // waves walk them at once --, also while they are still being filled: their hand-over records say "nothing to walk" beforehand.
            const uint32_t grid_side = (side_n + 3) / 4;   // (four of a workgroup's eight waves take pairs: one per SIMD, see k_small)
            grid_main = b->grid - grid_side;
            HIP_TRY(hipMemsetAsync(b->slot_info.p, 0xff, (size_t)side_n * sizeof(ba::SlotInfo), b->stream));
            HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
            BatchParams ps = p1;
            ps.n = side_n; ps.sm_excl_n = side_n; ps.sm_excl_first = 0;
            ps.work_counter = b->counter.as<uint32_t>() + 8;
            ps.big = (short*)((char*)b->big.p + (size_t)grid_main * ba::WAVES_PER_WG * ba::SM_WAVE_BYTES);
            ps.ckpt_wave0 = grid_main * ba::WAVES_PER_WG; ps.cq_side = 1;
            HIP_TRY(hipStreamWaitEvent(b->stream2, b->ev_fork, 0));
            HIP_TRY(kernel_launch(b, k, tr, grid_side, b->lds, b->stream2, &ps));
            HIP_TRY(hipEventRecord(b->ev_join, b->stream2));
            p1.sm_excl_first = side_n;
        }
        HIP_TRY(kernel_launch(b, k, tr, grid_main, b->lds, b->stream, &p1));
        if ((b->mode & BA_TRACE) && bp.cig_ops) {
            BatchParams pw = bp; pw.work_counter = b->counter.as<uint32_t>() + 16;   // (its own counters, zeroed with the others: the side launch may still be counting)
            if (special_of(b->mode)) HIP_TRY(ba_launch_walk_loc(b->stream, &pw, walk_grid(b)));   // (records with the zero-mask bits, the early stops)
            else HIP_TRY(ba_launch_walk_l2(b->stream, &pw, walk_grid(b)));
        }
        if (side_n) HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_join, 0));
    } else if (b->pipe) {   // pair-slot batch: the fill stacks, k_walk walks
        BatchParams p1 = bp; p1.cig_ops = nullptr; p1.inline_len2 = ~0u;
        HIP_TRY(kernel_launch(b, k, true, b->grid, b->lds, b->stream, &p1));
        if (bp.cig_ops) {
            HIP_TRY(hipMemsetAsync(b->counter.p, 0, 64, b->stream));
            HIP_TRY(ba_launch_walk(b->stream, &bp, walk_grid(b)));
        }
    } else
    HIP_TRY(kernel_launch(b, k, tr, b->grid, b->lds, b->stream, &bp));
    HIP_TRY(hipEventRecord(b->ev1, b->stream));
    b->in_flight = true;
    return 0;
}
template <class T>
static int d2h(const DevBuf& buf, T* dst, size_t count) {
    if (!dst) return 0;
    HIP_TRY(hipMemcpy(dst, buf.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
// Re-run the pairs `idx` (device order) of a TRACE batch with trace slots of the reference's full bound and put their results
// where the first pass left BA_ST_TRACE_OVERFLOW. The sub-batch reads the parent's resident images and matrix.
static int batch_retry(BaBatch* b, const std::vector<uint32_t>& idx, float* retry_ms) {
    const size_t k = idx.size(), n = b->n;
    std::vector<uint32_t> ql(n), rl(n);
    if (d2h(b->q_len, ql.data(), n) || d2h(b->r_len, rl.data(), n)) return 1;
    BaBatch sub;
    sub.device = b->device; sub.kind = b->kind; sub.mode = b->mode; sub.n = (uint32_t)k; sub.min_size = b->min_size; sub.max_size = b->max_size;
    sub.pclass = b->opt_class ? (uint32_t)BA_PCLASS_BIG : b->pclass; sub.gap_open = b->gap_open; sub.gap_extend = b->gap_extend; sub.x_drop = b->x_drop;
    sub.pad_negative = b->pad_negative;
    std::vector<uint64_t> qo(k), ro(k), co(k + 1);
    std::vector<uint32_t> sql(k), srl(k);
    uint64_t maxlen2 = 0, cig_total = 0;
    for (size_t t = 0; t < k; t++) {
        const uint32_t p = idx[t];
        qo[t] = b->h_q_off[p]; ro[t] = b->h_r_off[p]; sql[t] = ql[p]; srl[t] = rl[p];
        maxlen2 = std::max<uint64_t>(maxlen2, (uint64_t)ql[p] + rl[p] + 2);
        co[t] = cig_total; cig_total += (uint64_t)ql[p] + rl[p] + 1;
    }
    co[k] = cig_total;
    if (hipStreamCreateWithFlags(&sub.stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    if (hipEventCreate(&sub.ev0) != hipSuccess || hipEventCreate(&sub.ev1) != hipSuccess || hipEventCreate(&sub.ev_l0) != hipSuccess ||
        hipEventCreate(&sub.ev_m1) != hipSuccess) return fail("hipEventCreate failed");
    if (batch_plan(&sub, k, cig_total * 4 + (uint64_t)k * 64, maxlen2, true)) return 1;
    sub.cig_total = cig_total;
    sub.pool.view(b->pool.p, b->pool.bytes); sub.matrix.view(b->matrix.p, b->matrix.bytes);
    DevBuf d_idx;
    if (sub.q_off.alloc(k * 8) || sub.q_len.alloc(k * 4) || sub.r_off.alloc(k * 8) || sub.r_len.alloc(k * 4) || sub.cig_off.alloc((k + 1) * 8) ||
        sub.score.alloc(k * 4) || sub.qidx.alloc(k * 4) || sub.ridx.alloc(k * 4) || sub.cig_len.alloc(k * 4) || sub.cells.alloc(k * 8) ||
        sub.status.alloc(k * 4) || sub.nblocks.alloc(k * 4) || sub.pair_slot.alloc(k * 4) || sub.trace_words.alloc(k * 4) ||
        sub.cig_ops.alloc(cig_total * 4) || d_idx.alloc(k * 4) || batch_alloc_scratch(&sub)) return 1;
    HIP_TRY(hipMemcpy(sub.q_off.p, qo.data(), k * 8, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(sub.q_len.p, sql.data(), k * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sub.r_off.p, ro.data(), k * 8, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(sub.r_len.p, srl.data(), k * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sub.cig_off.p, co.data(), (k + 1) * 8, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(d_idx.p, idx.data(), k * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(sub.cig_len.p, 0, k * 4)); HIP_TRY(hipMemset(sub.status.p, 0, k * 4));
    if (batch_launch(&sub)) return 1;
    HIP_TRY(hipStreamSynchronize(sub.stream));
    sub.in_flight = false;
    const BatchParams sp = sub.params(), dp = b->params();
    HIP_TRY(hipEventRecord(sub.ev0, sub.stream));
    HIP_TRY(ba_launch_merge_retry(sub.stream, d_idx.as<uint32_t>(), (uint32_t)k, &sp, &dp, sub.trace_words.as<uint32_t>(), b->trace_words.as<uint32_t>()));
    HIP_TRY(hipEventRecord(sub.ev_m1, sub.stream));
    HIP_TRY(hipStreamSynchronize(sub.stream));
    // the re-run belongs to the batch's device time: its kernels (ev0 .. ev1 of the sub-batch's launch) and the merge
    if (retry_ms) {
        float a = 0, c = 0;
        HIP_TRY(hipEventElapsedTime(&a, sub.ev_l0, sub.ev1));
        HIP_TRY(hipEventElapsedTime(&c, sub.ev0, sub.ev_m1));
        *retry_ms = a + c;
    }
    return 0;
}
// The kernels wait for each other without a give-up (a fill wave for a trace slot, a traceback lane for a ring entry: round 4), so a hand-off that
// were ever lost would hang the launch: the host side bounds the wait instead (round-4 advisor finding) -- the launch is polled, and after
// g_wait_limit_ms (ba_set_wait_limit_ms; default 10 minutes, 0 = wait for ever) the call fails with a message instead of never returning.
static std::atomic<uint64_t> g_wait_limit_ms{600000};
void ba_set_wait_limit_ms(uint64_t ms) { g_wait_limit_ms.store(ms); }
// Returns 0 = done, 1 = the stream reported an error, 2 = the limit passed and the launch is STILL RUNNING (round-5 advisor finding: a timeout is not a
// failed launch -- the batch stays "in flight": results and a relaunch are refused until a later wait succeeds; ba_batch_destroy blocks in hipFree
// until the device lets go).
static int stream_wait_bounded(hipStream_t s, const char* what) {
    const uint64_t limit = g_wait_limit_ms.load();
    if (!limit) { HIP_TRY(hipStreamSynchronize(s)); return 0; }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 0;; spins++) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return fail("%s: %s", what, hipGetErrorString(e));
        if (spins < 256) continue;                                   // (short launches: the first polls back to back)
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (std::chrono::duration_cast<std::chrono::milliseconds>(dt).count() > (long long)limit) {
            fail("%s: the launch did not finish within %llu ms (ba_set_wait_limit_ms) and is still running: wait again, or the device may be hung", what, (unsigned long long)limit);
            return 2;
        }
        if (dt > std::chrono::microseconds(200)) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}
static int batch_wait(BaBatch* b, float* kernel_ms) {
    if (!b->in_flight) return fail("nothing was launched on this batch");
    HIP_TRY(hipSetDevice(b->device));
    if (const int w = stream_wait_bounded(b->stream, "ba_batch_wait")) {
        if (w != 2) b->in_flight = false;   // (a stream error ends the launch; a timeout does not: the batch stays in flight)
        return 1;
    }
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, b->ev0, b->ev1));
    b->in_flight = false;
    b->retried = 0;
    if (b->quad) {
        uint32_t ctl[64] = {0};
        HIP_TRY(hipMemcpy(ctl, b->cq_ctrl.p, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[48]) return fail("a per-pair kernel gave up waiting for the small-block kernel's queue");
        // every queued pair was taken by a per-pair wave: positions handed out (head) cover the entries appended (tail)
        if (ctl[16] < ctl[0]) return fail("small-block pipeline: %u queued pairs were never taken by the per-pair kernel", ctl[0] - ctl[16]);
    }
    if (b->adaptive || b->opt_class) {   // pairs whose trace stack outgrew the expected size: once more, with the reference's full bound
        // (... and, round 6, pairs whose block outgrew the launch's class: once more in the row-tiled class, opt_class)
        std::vector<uint32_t> st(b->n), again;
        if (d2h(b->status, st.data(), b->n)) return 1;
        for (uint32_t p = 0; p < b->n; p++) if (st[p] & (BA_ST_TRACE_OVERFLOW | ba::ST_CLASS_OVERFLOW)) again.push_back(p);
        if (b->opt_class) {
            size_t grew = 0;
            for (uint32_t p : again) if (st[p] & ba::ST_CLASS_OVERFLOW) grew++;
            if (grew * 8 > b->n && !dev_env("BA_KEEP_CLASS_BET")) b->bet_lost = true;
        }
        if (!again.empty()) {
            float retry_ms = 0;
            if (batch_retry(b, again, &retry_ms)) return 1;
            if (kernel_ms) *kernel_ms += retry_ms;   // the merged results include the re-run pairs' cells: so does the time
            b->retried = (uint32_t)again.size();
        }
    }
    b->ran = true;
    b->runs_done++;
    return 0;
}
static int batch_run(BaBatch* b, float* kernel_ms) {
    if (batch_launch(b)) return 1;
    return batch_wait(b, kernel_ms);
}


// dst holds one value per pair in device order: rearrange to the caller's order (dst[order[s]] = value of device entry s)
template <class T>
static void to_caller_order(const std::vector<uint32_t>& order, T* dst) {
    if (!dst || order.empty()) return;
    std::vector<T> tmp(dst, dst + order.size());
    for (size_t s = 0; s < order.size(); s++) dst[order[s]] = tmp[s];
}

template <class T>
static int h2d(DevBuf& buf, const T* src, size_t count) {
    HIP_TRY(hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// ------------------------------------------------------------------ objects that own a stream and events
// The device, one non-blocking stream and the timing events of an object with kernels of its own: extension and chain batches, the
// chainer, the seeder, an index build. A struct derived from it destroys its own members first: inner batches go before the outer stream.
namespace {   // (this and the other shared parts below add no name to the library's exports)
struct StreamOwner {
    int device = 0;
    hipStream_t stream = nullptr; hipEvent_t ev[9] = {};
    int open(size_t n_events) {
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
        for (size_t i = 0; i < n_events; i++) if (hipEventCreate(&ev[i]) != hipSuccess) return fail("hipEventCreate failed");
        return 0;
    }
    int elapsed(int a, int b, float* ms) const {   // device time between two recorded events
        HIP_TRY(hipEventElapsedTime(ms, ev[a], ev[b]));
        return 0;
    }
    ~StreamOwner() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ------------------------------------------------------------------ spliced batches: what extension and chain batches share
// Both are made of ordinary batches (batch_build: same planning, kernels and re-runs) over pieces that k_pack_images cuts out of the
// caller's bytes on the device -- uploaded once, no slice copied on the host --, and a splice that joins the pieces' results and CIGAR
// runs per unit (seed, chain) on the device, in the caller's order.
constexpr uint32_t NO_PIECE = 0xffffffffu;   // in an index of pieces: the piece is empty and was not aligned
static_assert(ba::EXT_NO_SIDE == NO_PIECE && ba::CHAIN_NO_PIECE == NO_PIECE, "EXT_NO_SIDE and CHAIN_NO_PIECE must both be 0xffffffff");
struct PieceSet {   // the pairs of one inner batch (host addresses into the caller's pool; nothing is copied)
    std::vector<const uint8_t*> src;   // 2 per piece (query, reference): first byte of the slice
    std::vector<uint32_t> len;         // 2 per piece
    std::vector<uint8_t> flags;        // 2 per piece: ba::IMG_*
    std::vector<uint32_t> owner;       // per piece: its seed or chain
    size_t size() const { return owner.size(); }
    uint32_t add(size_t u, const uint8_t* qs, uint64_t ql, uint8_t qf, const uint8_t* rs, uint64_t rl, uint8_t rf) {
        owner.push_back((uint32_t)u);
        src.push_back(qs); len.push_back((uint32_t)ql); flags.push_back(qf);
        src.push_back(rs); len.push_back((uint32_t)rl); flags.push_back(rf);
        return (uint32_t)owner.size() - 1;
    }
};
struct SplicedSet {   // a planned set: the extent of its sequences in the caller's pool, the size of the units' own images (seeds, anchors)
    const uint8_t* lo = nullptr; const uint8_t* hi = nullptr;
    uint64_t bytes = 0, own_bytes = 0;
    // per unit, the whole query and reference: source offsets in the upload, lengths, strand (ba_*_batch_text renders from them)
    std::vector<uint64_t> t_raw_q, t_raw_r;
    std::vector<uint32_t> t_ql, t_rl;
    std::vector<uint8_t> t_strand;
    void text_sources(const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, const uint8_t* strand, size_t n) {
        t_raw_q.assign(q_off, q_off + n); t_raw_r.assign(r_off, r_off + n); t_ql.assign(q_len, q_len + n); t_rl.assign(r_len, r_len + n);   // (made relative to lo by close)
        t_strand.assign(n, 0);
        if (strand) t_strand.assign(strand, strand + n);
    }
    // unit u (`noun`: "seed", "chain") on strand st: the strand checked, its sequences q and r added to the extent
    int add(int kind, const char* noun, size_t u, uint8_t st, const uint8_t* q, uint64_t Q, const uint8_t* r, uint64_t R) {
        if (st > 1) return fail("%s %zu: strand must be 0 or 1", noun, u);
        if (st && kind != BA_KIND_NUC) return fail("%s %zu: strand needs a NucMatrix batch (reverse complement is nucleotide-only)", noun, u);
        for (const uint8_t* x : {q, r}) if (!lo || x < lo) lo = x;
        if (!hi || q + Q > hi) hi = q + Q;
        if (r + R > hi) hi = r + R;
        return 0;
    }
    uint64_t own_image(uint64_t L) {   // -> the offset of one more own image of L bytes
        const uint64_t at = own_bytes;
        own_bytes += (1 + L + 3) & ~(uint64_t)3;
        return at;
    }
    uint64_t close(const uint8_t* pool) {   // after the last unit -> the offset of `lo` in the caller's pool
        bytes = (uint64_t)(hi - lo);
        const uint64_t base = (uint64_t)(lo - pool);
        for (uint64_t& x : t_raw_q) x -= base;
        for (uint64_t& x : t_raw_r) x -= base;
        return base;
    }
};
struct Spliced : StreamOwner {
    int kind = 0; uint32_t mode = 0, n = 0;
    uint64_t cap_n = 0, cap_raw = 0, cap_own = 0, runs_cap = 0, total_runs = 0;
    DevBuf raw, matrix, err;
    DevBuf score, left_score, right_score, q_start, r_start, q_end, r_end, cells, status, cigar_len, out_off, runs;
    float pack_ms = 0, splice_ms = 0;
    bool ran = false;
    DevBuf stats;   // per-unit statistics (ba_*_batch_stats), allocated on the first call
    float stats_ms = 0;   // ... the kernels of the last call (the inner batches' k_stats and the combine)
    // alignment strings (ba_*_batch_text): the sequences' source offsets, lengths and strands of the loaded set (host copies, uploaded by
    // the first text call after a load) and their device buffers, allocated on the first call
    std::vector<uint64_t> h_t_raw_q, h_t_raw_r;
    std::vector<uint32_t> h_t_ql, h_t_rl;
    std::vector<uint8_t> h_t_strand;
    bool t_uploaded = false;
    DevBuf t_raw_q, t_raw_r, t_ql, t_rl, t_strand;
    TextState text;
    uint64_t runs_done = 0;
    void text_loaded(const SplicedSet& S) {   // a set has been loaded: its sequences are what the next text call renders from
        h_t_raw_q = S.t_raw_q; h_t_raw_r = S.t_raw_r; h_t_ql = S.t_ql; h_t_rl = S.t_rl; h_t_strand = S.t_strand;
        t_uploaded = false;
    }
};
}  // namespace
// ba_*_batch_create's own arguments. what: "extension" / "chain"; the two sentences that differ are passed in.
static int spliced_check_params(const char* what, const char* cannot_be, const char* x_drop_why, int kind, Gaps gaps, SizeRange size, int32_t x_drop,
                                uint32_t mode) {
    if (kind == BA_KIND_PROFILE_) return fail("%s batches take a sequence matrix: profile batches cannot be %s", what, cannot_be);
    if (kind < 0 || kind > 2) return fail("unknown matrix kind %d", kind);
    if (!(mode & BA_X_DROP)) return fail("%s batches need BA_X_DROP: %s", what, x_drop_why);
    if (mode & (BA_LOCAL_START | BA_FREE_QUERY_START_GAPS | BA_FREE_QUERY_END_GAPS))
        return fail("%s batches take BA_X_DROP, BA_TRACE and BA_CIGAR_EQ only: LOCAL_START and FREE_QUERY_* are rejected", what);
    const size_t min_size = size.min < 16 ? 16 : size.min, max_size = size.max < 16 ? 16 : size.max;   // (as batch_build)
    std::string why;
    if (check_align_params(false, gaps, min_size, max_size, x_drop, mode, &why)) return fail("%s", why.c_str());
    if (min_size > max_size) return fail("min block size exceeds max block size");
    return 0;
}
// create, before the object's own buffers: the capacities are this set's; the caller's bytes, the pool of the units' own images, the error word
static int spliced_create_head(Spliced* e, const SplicedSet& S, size_t n, DevBuf& own_pool) {
    e->cap_n = n; e->cap_raw = S.bytes; e->cap_own = S.own_bytes;
    return e->raw.alloc(S.bytes) || own_pool.alloc(S.own_bytes + 64) || e->err.alloc(8);
}
// create, after them: the last shared buffers and the matrix (1024 bytes, as batch_build lays it out)
static int spliced_create_tail(Spliced* e, size_t n, const void* matrix) {
    if (e->cells.alloc(n * 8) || e->out_off.alloc((n + 1) * 8) || e->matrix.alloc(1024)) return 1;
    int8_t tmp[1024] = {0};
    if (e->kind == BA_KIND_BYTES) { const ByteMatrix* bm = (const ByteMatrix*)matrix; tmp[0] = bm->match_score; tmp[1] = bm->mismatch_score; }
    else memcpy(tmp, matrix, e->kind == BA_KIND_AA ? 27 * 32 : 8 * 16);
    return h2d(e->matrix, tmp, 1024);
}
// reload: what the set may not exceed. They return before anything is cleared: the earlier set stays loaded.
static int over_count(const char* nouns, size_t n, uint64_t cap) {
    return n > cap ? fail("reload: %zu %s exceed the batch's capacity of %llu", n, nouns, (unsigned long long)cap) : 0;
}
static int over_bytes(const Spliced* e, const SplicedSet& S, const char* own) {
    if (S.bytes > e->cap_raw) return fail("reload: %llu sequence bytes exceed the batch's capacity of %llu", (unsigned long long)S.bytes, (unsigned long long)e->cap_raw);
    if (S.own_bytes > e->cap_own) return fail("reload: the %s (%llu image bytes) exceed the batch's capacity of %llu", own, (unsigned long long)S.own_bytes, (unsigned long long)e->cap_own);
    return 0;
}
static int no_inner(const char* pieces, const PieceSet& P, const std::unique_ptr<BaBatch>& inner) {
    return P.size() && !inner ? fail("reload: the set has %s to align, and the batch was created with none", pieces) : 0;
}
// The pieces of one inner batch into it (built on create, reloaded after); `side`: the pieces' indices -> their positions in its device
// order. what: what a piece belongs to ("seed", "chain"), for the message about a byte outside the alphabet.
static int spliced_load_pieces(Spliced* e, std::unique_ptr<BaBatch>& inner, const PieceSet& P, const uint8_t* lo, const char* what, const void* matrix,
                               Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, bool create, std::vector<uint32_t>& side) {
    const size_t np = P.size();
    if (!np) return 0;
    float ms = 0;
    ExtImages X;
    X.host_base = lo; X.dev_base = e->raw.as<uint8_t>(); X.flags = P.flags.data(); X.seed_of = P.owner.data(); X.pack_ms = &ms; X.what = what;
    auto get = [&](size_t p, int w, const uint8_t** ptr, size_t* len) { *ptr = P.src[2 * p + w]; *len = P.len[2 * p + w]; };
    if (create) {
        inner.reset(batch_build(e->kind, matrix, gaps, size, x_drop, mode, np, false, get, NoProfiles(), &X));
        if (!inner) return 1;
    } else if (batch_reload(inner.get(), np, false, get, NoProfiles(), &X)) return 1;
    e->pack_ms += ms;
    if (!inner->h_order.empty()) {
        std::vector<uint32_t> pos(np);
        for (uint32_t d = 0; d < np; d++) pos[inner->h_order[d]] = d;
        for (uint32_t& x : side) if (x != NO_PIECE) x = pos[x];
    }
    return 0;
}
// The units' own images (n seeds or anchors; their six arrays are on the device): k_pack_images timed, its time added to pack_ms
// -> *err: the kernel's error word, ~0 if every byte is in the alphabet
static int spliced_pack_own(Spliced* e, const DevBuf& raw_q, const DevBuf& raw_r, const DevBuf& flags, const DevBuf& img_q, const DevBuf& img_r,
                            const DevBuf& len, const DevBuf& pool, size_t n, unsigned long long* err) {
    HIP_TRY(hipMemset(e->err.p, 0xff, 8));
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    HIP_TRY(ba_launch_pack_images(e->stream, seq_kind(e->kind), e->raw.as<uint8_t>(), raw_q.as<uint64_t>(), raw_r.as<uint64_t>(), flags.as<uint8_t>(),
                                  img_q.as<uint64_t>(), len.as<uint32_t>(), img_r.as<uint64_t>(), len.as<uint32_t>(), pool.as<uint8_t>(), 0, (uint32_t)n,
                                  e->err.as<unsigned long long>()));
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (e->elapsed(0, 1, &ms)) return 1;
    e->pack_ms += ms;
    return d2h(e->err, err, 1);
}
// The splice behind the fills: `results` launched and timed; with TRACE the total of the runs read, `runs` grown to it, `gather` launched
// and timed (it reads e->runs afresh: the buffer may have moved).
template <class Results, class Gather>
static int spliced_splice(Spliced* e, Results results, Gather gather) {
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    HIP_TRY(results());
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->elapsed(0, 1, &e->splice_ms)) return 1;
    if (e->mode & BA_TRACE) {
        uint64_t total = 0;
        HIP_TRY(hipMemcpy(&total, e->out_off.as<uint64_t>() + e->n, 8, hipMemcpyDeviceToHost));
        if (total > e->runs_cap) {
            if (e->runs.alloc(total * 4)) return 1;
            e->runs_cap = total;
        }
        HIP_TRY(hipEventRecord(e->ev[2], e->stream));
        HIP_TRY(gather());
        HIP_TRY(hipEventRecord(e->ev[3], e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        float ms = 0;
        if (e->elapsed(2, 3, &ms)) return 1;
        e->splice_ms += ms;
        e->total_runs = total;
    }
    e->ran = true;
    return 0;
}
// ba_*_batch_results and ba_*_batch_cigars. call: "extend_batch" / "chain_batch".
static int spliced_results(Spliced* e, const char* call, int32_t* score, uint32_t* q_start, uint32_t* r_start, uint32_t* q_end, uint32_t* r_end,
                           int32_t* left_score, int32_t* right_score, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_%s_run has not been called", call);
    HIP_TRY(hipSetDevice(e->device));
    if (d2h(e->score, score, e->n) || d2h(e->q_start, q_start, e->n) || d2h(e->r_start, r_start, e->n) || d2h(e->q_end, q_end, e->n) ||
        d2h(e->r_end, r_end, e->n) || d2h(e->left_score, left_score, e->n) || d2h(e->right_score, right_score, e->n) ||
        d2h(e->cells, cells, e->n) || d2h(e->cigar_len, cigar_len, e->n) || d2h(e->status, status, e->n)) return 1;
    return 0;
}
static int spliced_cigars(Spliced* e, const char* call, uint32_t* runs, uint64_t capacity) {
    if (!e) return fail("null batch");
    if (!(e->mode & BA_TRACE)) return fail("batch was created without BA_TRACE");
    if (!e->ran) return fail("ba_%s_run has not been called", call);
    if (e->total_runs > capacity) return fail("cigar buffer too small: need %llu entries", (unsigned long long)e->total_runs);
    if (!e->total_runs) return 0;
    if (!runs) return fail("null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(runs, e->runs.p, e->total_runs * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ seed-and-extend batches (ba_extend_batch_*)
// One seed = one result: X-drop alignment leftwards from the seed (reversed prefixes) and rightwards from its end. Every non-empty side of
// every seed is a pair of ONE ordinary batch, the seeds' own images are packed beside them; the splice (ba_extend.hip) then scores the
// seeds and joins both sides' results and CIGAR runs per seed.
struct ExtSet : SplicedSet {   // a seed set cut into sides
    PieceSet sides;
    std::vector<uint32_t> side;                        // 2 per seed (left, right): index of the side, or NO_PIECE
    std::vector<uint64_t> s_raw_q, s_raw_r, s_img_q, s_img_r;   // the seeds' own images: source offsets in the upload, offsets in the seed pool
    std::vector<uint8_t> s_flags;                      // 2 per seed
};
// Check a seed set (the mode and the matrix kind are checked already) and cut it into sides.
static int ext_plan(int kind, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                    const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, const uint8_t* strand, size_t n, ExtSet& S) {
    if (!pool || !q_off || !q_len || !r_off || !r_len || !q_seed || !r_seed || !seed_len) return fail("null argument");
    if (n == 0 || n > (1u << 28)) return fail("an extension batch must hold between 1 and 2^28 seeds");   // (k_pack_images: two workgroups per side)
    S = ExtSet();
    S.side.resize(2 * n); S.s_raw_q.resize(n); S.s_raw_r.resize(n); S.s_img_q.resize(n); S.s_img_r.resize(n); S.s_flags.resize(2 * n);
    S.text_sources(q_off, q_len, r_off, r_len, strand, n);
    for (size_t p = 0; p < n; p++) {
        const uint64_t Q = q_len[p], R = r_len[p], s = q_seed[p], t = r_seed[p], L = seed_len[p];
        if (L == 0) return fail("seed %zu: seed_len must be at least 1", p);
        if (s + L > Q || t + L > R)
            return fail("seed %zu: the seed (query %llu + %llu, reference %llu + %llu) runs past the end of its sequences (%llu, %llu)", p,
                        (unsigned long long)s, (unsigned long long)L, (unsigned long long)t, (unsigned long long)L, (unsigned long long)Q, (unsigned long long)R);
        const uint8_t st = strand ? strand[p] : 0;
        const uint8_t* q = pool + q_off[p]; const uint8_t* r = pool + r_off[p];
        if (S.add(kind, "seed", p, st, q, Q, r, R)) return 1;
        auto add_side = [&](int w, const uint8_t* qs, uint64_t ql, uint8_t qf, const uint8_t* rs, uint64_t rl, uint8_t rf) {
            S.side[2 * p + w] = ql && rl ? S.sides.add(p, qs, ql, qf, rs, rl, rf) : NO_PIECE;
        };
        // (minus strand: q is the reverse complement of the caller's bytes; the seed's frame is that of q)
        if (st) add_side(0, q + (Q - s), s, ba::IMG_COMPLEMENT, r, t, ba::IMG_REVERSE);
        else add_side(0, q, s, ba::IMG_REVERSE, r, t, ba::IMG_REVERSE);
        if (st) add_side(1, q, Q - s - L, ba::IMG_REVERSE | ba::IMG_COMPLEMENT, r + t + L, R - t - L, 0);
        else add_side(1, q + s + L, Q - s - L, 0, r + t + L, R - t - L, 0);
        S.s_raw_q[p] = (uint64_t)((st ? q + (Q - s - L) : q + s) - pool); S.s_raw_r[p] = (uint64_t)(r + t - pool);   // (made relative to lo below)
        S.s_flags[2 * p] = st ? (ba::IMG_REVERSE | ba::IMG_COMPLEMENT) : 0; S.s_flags[2 * p + 1] = 0;
        S.s_img_q[p] = S.own_image(L); S.s_img_r[p] = S.own_image(L);
    }
    const uint64_t base = S.close(pool);
    for (size_t p = 0; p < n; p++) { S.s_raw_q[p] -= base; S.s_raw_r[p] -= base; }
    if (S.sides.size() > 0x7fffffffu) return fail("too many sides");
    return 0;
}
struct BaExtendBatch : Spliced {
    std::unique_ptr<BaBatch> inner;   // the sides of the loaded set; null if the batch was created with none (nothing to fill)
    uint32_t n_sides = 0;
    DevBuf seed_pool, seed_q, seed_r, seed_raw_q, seed_raw_r, seed_flags, seed_len, q_seed, r_seed, side, join;
    float fill_ms = 0;
    // optimal paths (ba_extend_batch_exact_paths): the requested seeds, their run counts, offsets and joined runs on the device, and the
    // request they belong to with its records, kept for the second call of the two-call pattern (a load drops it)
    DevBuf xp_sel, xp_nrun, xp_off, xp_runs, xp_seed, xp_no_off;   // (xp_seed: the seeds' ungapped scores; xp_no_off: zero offsets for a set without sides)
    bool xp_valid = false; int32_t xp_x_drop = 0;
    std::vector<uint32_t> xp_which; std::vector<BaExactPath> xp_out; std::vector<BaExact> xp_left, xp_right; std::vector<uint64_t> xp_h_off;
    ba::ExtendParams params() const {
        ba::ExtendParams ep{};
        ep.n = n; ep.kind = seq_kind(kind); ep.flags = mode; ep.matrix = matrix.as<int8_t>();
        ep.q_seed = q_seed.as<uint32_t>(); ep.r_seed = r_seed.as<uint32_t>(); ep.seed_len = seed_len.as<uint32_t>();
        ep.seed_pool = seed_pool.as<uint8_t>(); ep.seed_q = seed_q.as<uint64_t>(); ep.seed_r = seed_r.as<uint64_t>(); ep.side = side.as<uint32_t>();
        if (inner) {
            const BaBatch* b = inner.get();
            ep.in_score = b->score.as<int32_t>(); ep.in_qidx = b->qidx.as<uint32_t>(); ep.in_ridx = b->ridx.as<uint32_t>();
            ep.in_cells = b->cells.as<unsigned long long>(); ep.in_status = b->status.as<uint32_t>(); ep.in_cig_len = b->cig_len.as<uint32_t>();
            ep.in_cig_off = b->cig_off.as<uint64_t>(); ep.in_cig_ops = b->cig_ops.as<uint32_t>();
        }
        ep.score = score.as<int32_t>(); ep.left_score = left_score.as<int32_t>(); ep.right_score = right_score.as<int32_t>();
        ep.q_start = q_start.as<uint32_t>(); ep.r_start = r_start.as<uint32_t>(); ep.q_end = q_end.as<uint32_t>(); ep.r_end = r_end.as<uint32_t>();
        ep.cells = cells.as<unsigned long long>(); ep.status = status.as<uint32_t>(); ep.cigar_len = cigar_len.as<uint32_t>();
        ep.join = join.as<uint32_t>(); ep.out_off = out_off.as<uint64_t>(); ep.runs = runs.as<uint32_t>();
        return ep;
    }
};
// Load a planned set into the batch: the caller's bytes once to the device, the sides into the inner batch (built on create, reloaded
// after), the seeds' own images. `create`: size every buffer for this set; otherwise the set must fit them.
static int ext_load(BaExtendBatch* e, const ExtSet& S, size_t n, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop,
                    const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, bool create) {
    if (create) {
        if (spliced_create_head(e, S, n, e->seed_pool)) return 1;
        DevBuf* per_seed4[] = {&e->seed_len, &e->q_seed, &e->r_seed, &e->score, &e->left_score, &e->right_score, &e->q_start, &e->r_start,
                               &e->q_end, &e->r_end, &e->status, &e->cigar_len, &e->join};
        for (DevBuf* d : per_seed4) if (d->alloc(n * 4)) return 1;
        if (e->seed_q.alloc(n * 8) || e->seed_r.alloc(n * 8) || e->seed_raw_q.alloc(n * 8) || e->seed_raw_r.alloc(n * 8) || e->seed_flags.alloc(2 * n) ||
            e->side.alloc(2 * n * 4) || spliced_create_tail(e, n, matrix)) return 1;
    } else if (over_count("seeds", n, e->cap_n) || over_bytes(e, S, "seeds") || no_inner("sides", S.sides, e->inner)) return 1;
    e->n = 0; e->ran = false; e->pack_ms = 0; e->xp_valid = false;   // (a failure from here on leaves no seeds loaded)
    if (h2d(e->raw, S.lo, S.bytes)) return 1;
    std::vector<uint32_t> side(S.side);
    if (spliced_load_pieces(e, e->inner, S.sides, S.lo, "seed", matrix, gaps, size, x_drop, e->mode, create, side)) return 1;
    if (h2d(e->side, side.data(), 2 * n) || h2d(e->q_seed, q_seed, n) || h2d(e->r_seed, r_seed, n) || h2d(e->seed_len, seed_len, n) ||
        h2d(e->seed_q, S.s_img_q.data(), n) || h2d(e->seed_r, S.s_img_r.data(), n) || h2d(e->seed_raw_q, S.s_raw_q.data(), n) ||
        h2d(e->seed_raw_r, S.s_raw_r.data(), n) || h2d(e->seed_flags, S.s_flags.data(), 2 * n)) return 1;
    HIP_TRY(hipMemset(e->cigar_len.p, 0, n * 4));
    unsigned long long err = 0;
    if (spliced_pack_own(e, e->seed_raw_q, e->seed_raw_r, e->seed_flags, e->seed_q, e->seed_r, e->seed_len, e->seed_pool, n, &err)) return 1;
    if (err != ~0ull) return fail("seed %llu: byte 0x%02x is outside the matrix alphabet", err >> 8, (unsigned)(err & 0xff));
    e->n = (uint32_t)n; e->n_sides = (uint32_t)S.sides.size();
    e->text_loaded(S);
    return 0;
}

// ------------------------------------------------------------------ anchor-chain batches (ba_chain_batch_*)
// One chain of colinear anchors = one result: X-drop extension leftwards from the first anchor and rightwards from the last one, as for a
// seed; a global alignment of the slices between consecutive anchors; the anchors themselves ungapped. The ends of every chain are the pairs
// of ONE X-drop batch, the gaps with two non-empty slices the pairs of ONE global batch; the segmented splice (ba_chain.hip) scores the
// anchors, makes the runs of the gaps with one empty slice and joins everything per chain.
struct ChainSet : SplicedSet {   // a set of chains cut into pieces
    PieceSet ends, gaps;
    std::vector<uint32_t> end_side;                    // 2 per chain (left, right): index of the end in `ends`, or NO_PIECE
    std::vector<uint32_t> gap_side;                    // per anchor: index in `gaps` of the gap behind it, or NO_PIECE
    std::vector<uint64_t> a_raw_q, a_raw_r, a_img_q, a_img_r;   // the anchors' own images: source offsets in the upload, offsets in the anchor pool
    std::vector<uint8_t> a_flags;                      // 2 per anchor
    uint64_t n_anchors = 0;
};
// Check a set of chains (the mode and the matrix kind are checked already) and cut it into ends, gaps and anchors.
static int chain_plan(int kind, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                      const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len, const uint8_t* strand,
                      size_t n, ChainSet& S) {
    if (!pool || !q_off || !q_len || !r_off || !r_len || !anchor_first || !q_anchor || !r_anchor || !anchor_len) return fail("null argument");
    if (n == 0 || n > (1u << 28)) return fail("a chain batch must hold between 1 and 2^28 chains");
    if (anchor_first[0] != 0) return fail("anchor_first must start at 0 (chain 0 starts at %llu)", (unsigned long long)anchor_first[0]);
    for (size_t c = 0; c < n; c++) {
        if (anchor_first[c + 1] < anchor_first[c])
            return fail("chain %zu: anchor_first must not decrease (%llu after %llu)", c, (unsigned long long)anchor_first[c + 1], (unsigned long long)anchor_first[c]);
        if (anchor_first[c + 1] == anchor_first[c]) return fail("chain %zu: a chain must hold at least one anchor", c);
    }
    const uint64_t na = anchor_first[n];
    if (na > (1u << 28)) return fail("a chain batch must hold at most 2^28 anchors");   // (k_pack_images: two workgroups per anchor)
    S = ChainSet();
    S.n_anchors = na;
    S.text_sources(q_off, q_len, r_off, r_len, strand, n);
    S.end_side.resize(2 * n); S.gap_side.assign(na, NO_PIECE);
    S.a_raw_q.resize(na); S.a_raw_r.resize(na); S.a_img_q.resize(na); S.a_img_r.resize(na); S.a_flags.resize(2 * na);
    for (size_t c = 0; c < n; c++) {
        const uint64_t Q = q_len[c], R = r_len[c];
        const uint8_t st = strand ? strand[c] : 0;
        const uint8_t* q = pool + q_off[c]; const uint8_t* r = pool + r_off[c];
        if (S.add(kind, "chain", c, st, q, Q, r, R)) return 1;
        // (minus strand: q is the reverse complement of the caller's bytes, and a slice [a, b) of it the reversed, complemented slice
        // [Q - b, Q - a) of those bytes)
        const uint8_t fwd = st ? (ba::IMG_REVERSE | ba::IMG_COMPLEMENT) : 0;
        auto q_slice = [&](uint64_t a, uint64_t b) { return st ? q + (Q - b) : q + a; };
        const uint64_t a0 = anchor_first[c], K = anchor_first[c + 1] - a0;
        for (uint64_t k = 0; k < K; k++) {
            const uint64_t a = a0 + k, s = q_anchor[a], t = r_anchor[a], L = anchor_len[a];
            if (L == 0) return fail("chain %zu, anchor %llu: anchor_len must be at least 1", c, (unsigned long long)k);
            if (s + L > Q || t + L > R)
                return fail("chain %zu, anchor %llu: the anchor (query %llu + %llu, reference %llu + %llu) runs past the end of its sequences (%llu, %llu)", c,
                            (unsigned long long)k, (unsigned long long)s, (unsigned long long)L, (unsigned long long)t, (unsigned long long)L,
                            (unsigned long long)Q, (unsigned long long)R);
            if (k) {
                const uint64_t ps = (uint64_t)q_anchor[a - 1] + anchor_len[a - 1], pt = (uint64_t)r_anchor[a - 1] + anchor_len[a - 1];
                if (s < ps || t < pt)
                    return fail("chain %zu, anchor %llu: the anchor overlaps or precedes anchor %llu on the %s (it starts at %llu, anchor %llu ends at %llu)", c,
                                (unsigned long long)k, (unsigned long long)(k - 1), s < ps ? "query" : "reference", (unsigned long long)(s < ps ? s : t),
                                (unsigned long long)(k - 1), (unsigned long long)(s < ps ? ps : pt));
                if (s > ps && t > pt)   // both slices non-empty: a pair of the global batch (one empty: a single I or D run, made by the splice)
                    S.gap_side[a - 1] = S.gaps.add(c, q_slice(ps, s), s - ps, fwd, r + pt, t - pt, 0);
            }
            S.a_raw_q[a] = (uint64_t)(q_slice(s, s + L) - pool); S.a_raw_r[a] = (uint64_t)(r + t - pool);   // (made relative to lo below)
            S.a_flags[2 * a] = fwd; S.a_flags[2 * a + 1] = 0;
            S.a_img_q[a] = S.own_image(L); S.a_img_r[a] = S.own_image(L);
        }
        // the ends: the two sides of a seed (ext_plan), left of the first anchor and right of the last one
        const uint64_t s = q_anchor[a0], t = r_anchor[a0], al = a0 + K - 1, eq = (uint64_t)q_anchor[al] + anchor_len[al], er = (uint64_t)r_anchor[al] + anchor_len[al];
        S.end_side[2 * c] = (s && t) ? S.ends.add(c, st ? q + (Q - s) : q, s, st ? ba::IMG_COMPLEMENT : ba::IMG_REVERSE, r, t, ba::IMG_REVERSE) : NO_PIECE;
        S.end_side[2 * c + 1] = (Q - eq && R - er) ? S.ends.add(c, q_slice(eq, Q), Q - eq, fwd, r + er, R - er, 0) : NO_PIECE;
    }
    const uint64_t base = S.close(pool);
    for (uint64_t a = 0; a < na; a++) { S.a_raw_q[a] -= base; S.a_raw_r[a] -= base; }
    if (S.ends.size() > 0x7fffffffu || S.gaps.size() > 0x7fffffffu) return fail("too many pieces");
    return 0;
}
struct BaChainBatch : Spliced {
    int gap_open = 0, gap_extend = 0;
    std::unique_ptr<BaBatch> ends, gaps;   // the X-drop batch of the ends, the global batch of the gaps; null if the batch was created without such pieces
    uint32_t n_anchors = 0, n_ends = 0, n_gaps = 0;
    uint64_t cap_anchors = 0;
    DevBuf anchor_pool, anchor_q, anchor_r, anchor_raw_q, anchor_raw_r, anchor_flags, anchor_len, q_anchor, r_anchor, anchor_first, end_side, gap_side;
    DevBuf a_score, a_nrun, a_ops, a_flen, a_llen;
    float ends_ms = 0, gaps_ms = 0;
    static ba::ChainPieces pieces(const BaBatch* b) {
        ba::ChainPieces pc{};
        if (!b) return pc;
        pc.score = b->score.as<int32_t>(); pc.qidx = b->qidx.as<uint32_t>(); pc.ridx = b->ridx.as<uint32_t>();
        pc.cells = b->cells.as<unsigned long long>(); pc.status = b->status.as<uint32_t>(); pc.cig_len = b->cig_len.as<uint32_t>();
        pc.cig_off = b->cig_off.as<uint64_t>(); pc.cig_ops = b->cig_ops.as<uint32_t>();
        return pc;
    }
    ba::ChainParams params() const {
        ba::ChainParams cp{};
        cp.n = n; cp.n_anchors = n_anchors; cp.kind = seq_kind(kind); cp.flags = mode; cp.gap_open = gap_open; cp.gap_extend = gap_extend;
        cp.matrix = matrix.as<int8_t>(); cp.anchor_first = anchor_first.as<uint64_t>();
        cp.q_anchor = q_anchor.as<uint32_t>(); cp.r_anchor = r_anchor.as<uint32_t>(); cp.anchor_len = anchor_len.as<uint32_t>();
        cp.anchor_pool = anchor_pool.as<uint8_t>(); cp.anchor_q = anchor_q.as<uint64_t>(); cp.anchor_r = anchor_r.as<uint64_t>();
        cp.end_side = end_side.as<uint32_t>(); cp.gap_side = gap_side.as<uint32_t>();
        cp.ends = pieces(n_ends ? ends.get() : nullptr); cp.gaps = pieces(n_gaps ? gaps.get() : nullptr);
        cp.a_score = a_score.as<int32_t>(); cp.a_nrun = a_nrun.as<uint32_t>(); cp.a_ops = a_ops.as<uint32_t>();
        cp.a_flen = a_flen.as<uint32_t>(); cp.a_llen = a_llen.as<uint32_t>();
        cp.score = score.as<int32_t>(); cp.left_score = left_score.as<int32_t>(); cp.right_score = right_score.as<int32_t>();
        cp.q_start = q_start.as<uint32_t>(); cp.r_start = r_start.as<uint32_t>(); cp.q_end = q_end.as<uint32_t>(); cp.r_end = r_end.as<uint32_t>();
        cp.cells = cells.as<unsigned long long>(); cp.status = status.as<uint32_t>(); cp.cigar_len = cigar_len.as<uint32_t>();
        cp.out_off = out_off.as<uint64_t>(); cp.runs = runs.as<uint32_t>();
        return cp;
    }
};
// Load a planned set into the batch: the caller's bytes once to the device, the ends and the gaps into their inner batches, the anchors'
// own images. `create`: size every buffer for this set; otherwise the set must fit them.
static int chain_load(BaChainBatch* e, const ChainSet& S, size_t n, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop,
                      const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len, bool create) {
    const size_t na = S.n_anchors;
    if (create) {
        e->cap_anchors = na;
        if (spliced_create_head(e, S, n, e->anchor_pool)) return 1;
        DevBuf* per_chain4[] = {&e->score, &e->left_score, &e->right_score, &e->q_start, &e->r_start, &e->q_end, &e->r_end, &e->status, &e->cigar_len};
        for (DevBuf* d : per_chain4) if (d->alloc(n * 4)) return 1;
        DevBuf* per_anchor4[] = {&e->anchor_len, &e->q_anchor, &e->r_anchor, &e->gap_side, &e->a_score, &e->a_nrun, &e->a_ops, &e->a_flen, &e->a_llen};
        for (DevBuf* d : per_anchor4) if (d->alloc(na * 4)) return 1;
        if (e->anchor_q.alloc(na * 8) || e->anchor_r.alloc(na * 8) || e->anchor_raw_q.alloc(na * 8) || e->anchor_raw_r.alloc(na * 8) || e->anchor_flags.alloc(2 * na) ||
            e->anchor_first.alloc((n + 1) * 8) || e->end_side.alloc(2 * n * 4) || spliced_create_tail(e, n, matrix)) return 1;
    } else if (over_count("chains", n, e->cap_n) || over_count("anchors", na, e->cap_anchors) || over_bytes(e, S, "anchors") ||
               no_inner("ends", S.ends, e->ends) || no_inner("gaps", S.gaps, e->gaps)) return 1;
    e->n = 0; e->ran = false; e->pack_ms = 0;   // (a failure from here on leaves no chains loaded)
    if (h2d(e->raw, S.lo, S.bytes)) return 1;
    std::vector<uint32_t> end_side(S.end_side), gap_side(S.gap_side);
    {
        // both inner batches live together: the first one plans with half of the free memory (as the ranges of ba_sized_batch_create share it)
        struct CapReset { ~CapReset() { g_mem_cap = ~0ull; } } cap_reset;
        if (create && S.ends.size() && S.gaps.size()) {
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            g_mem_cap = std::max<uint64_t>((uint64_t)((double)free_b * 0.95 * 0.5), 3ull << 30);
        }
        if (spliced_load_pieces(e, e->ends, S.ends, S.lo, "chain", matrix, gaps, size, x_drop, e->mode, create, end_side)) return 1;
        g_mem_cap = ~0ull;
        if (spliced_load_pieces(e, e->gaps, S.gaps, S.lo, "chain", matrix, gaps, size, 0, e->mode & ~(uint32_t)BA_X_DROP, create, gap_side)) return 1;
    }
    if (h2d(e->end_side, end_side.data(), 2 * n) || h2d(e->gap_side, gap_side.data(), na) || h2d(e->anchor_first, anchor_first, n + 1) ||
        h2d(e->q_anchor, q_anchor, na) || h2d(e->r_anchor, r_anchor, na) || h2d(e->anchor_len, anchor_len, na) ||
        h2d(e->anchor_q, S.a_img_q.data(), na) || h2d(e->anchor_r, S.a_img_r.data(), na) || h2d(e->anchor_raw_q, S.a_raw_q.data(), na) ||
        h2d(e->anchor_raw_r, S.a_raw_r.data(), na) || h2d(e->anchor_flags, S.a_flags.data(), 2 * na)) return 1;
    HIP_TRY(hipMemset(e->cigar_len.p, 0, n * 4));
    unsigned long long err = 0;
    if (spliced_pack_own(e, e->anchor_raw_q, e->anchor_raw_r, e->anchor_flags, e->anchor_q, e->anchor_r, e->anchor_len, e->anchor_pool, na, &err)) return 1;
    if (err != ~0ull) {
        const uint64_t a = err >> 8;
        const size_t c = (size_t)(std::upper_bound(anchor_first, anchor_first + n + 1, a) - anchor_first) - 1;
        return fail("chain %zu, anchor %llu: byte 0x%02x is outside the matrix alphabet", c, (unsigned long long)(a - anchor_first[c]), (unsigned)(err & 0xff));
    }
    e->n = (uint32_t)n; e->n_anchors = (uint32_t)na; e->n_ends = (uint32_t)S.ends.size(); e->n_gaps = (uint32_t)S.gaps.size();
    e->text_loaded(S);
    return 0;
}

// ------------------------------------------------------------------ per-alignment statistics (ba_*_stats)
// k_stats (ba_stats.hip) over a traced batch after its run: one record per pair into b->stats (allocated on the first call, freed with the
// batch), at the pair's caller-order position or -- the sides of an extension batch -- at its device position. The runs it reads are the
// final ones (re-runs are merged into the batch's arrays by ba_batch_wait).
static_assert(sizeof(BaAlignStats) == sizeof(ba::AlignStats) && offsetof(BaAlignStats, matches) == offsetof(ba::AlignStats, matches) &&
              offsetof(BaAlignStats, gap_opens) == offsetof(ba::AlignStats, gap_opens) && offsetof(BaAlignStats, path_score) == offsetof(ba::AlignStats, path_score),
              "BaAlignStats and ba::AlignStats differ");
static int batch_stats_device(BaBatch* b, bool caller_order) {
    if (!(b->mode & BA_TRACE)) return fail("stats: the batch was created without BA_TRACE (the statistics are computed from the CIGAR runs)");
    if (b->kind == BA_KIND_PROFILE_) return fail("stats: a profile batch has no reference bytes to compare with");
    if (b->in_flight) return fail("stats: the batch has a launch in flight (ba_batch_wait first)");
    if (!b->ran) return fail("stats: the batch has not finished a run (ba_batch_run, or ba_batch_launch and ba_batch_wait)");
    HIP_TRY(hipSetDevice(b->device));
    if (!b->stats.p && b->stats.alloc((size_t)b->cap_n * sizeof(ba::AlignStats))) return 1;
    const bool map = caller_order && !b->h_order.empty();
    if (map) {
        if (!b->stats_pos.p && b->stats_pos.alloc((size_t)b->cap_n * 4)) return 1;
        HIP_TRY(hipMemcpy(b->stats_pos.p, b->h_order.data(), (size_t)b->n * 4, hipMemcpyHostToDevice));
    }
    if (!b->ev_s0) HIP_TRY(hipEventCreate(&b->ev_s0));
    if (!b->ev_s1) HIP_TRY(hipEventCreate(&b->ev_s1));
    ba::StatsParams sp{};
    sp.n = b->n; sp.kind = seq_kind(b->kind); sp.gap_open = b->gap_open; sp.gap_extend = b->gap_extend;
    sp.matrix = b->matrix.as<int8_t>(); sp.matrix_bytes = (uint32_t)b->matrix.bytes;
    sp.pool = b->pool.as<uint8_t>(); sp.q_off = b->q_off.as<uint64_t>(); sp.q_len = b->q_len.as<uint32_t>();
    sp.r_off = b->r_off.as<uint64_t>(); sp.r_len = b->r_len.as<uint32_t>();
    sp.qidx = b->qidx.as<uint32_t>(); sp.ridx = b->ridx.as<uint32_t>(); sp.status = b->status.as<uint32_t>();
    sp.cig_len = b->cig_len.as<uint32_t>(); sp.cig_off = b->cig_off.as<uint64_t>(); sp.cig_ops = b->cig_ops.as<uint32_t>();
    sp.out_pos = map ? b->stats_pos.as<uint32_t>() : nullptr;
    sp.out = b->stats.as<ba::AlignStats>();
    HIP_TRY(hipEventRecord(b->ev_s0, b->stream));
    HIP_TRY(ba_launch_stats(b->stream, &sp));
    HIP_TRY(hipEventRecord(b->ev_s1, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipEventElapsedTime(&b->stats_ms, b->ev_s0, b->ev_s1));
    return 0;
}

// ------------------------------------------------------------------ exact full-matrix scores (ba_*_exact)
// k_exact (ba_exact.hip) over the images, matrix and gaps of a batch: no run is needed and none is read. The request is a list of device
// positions (EXACT_NO_PAIR: an all-zero record); it is sorted by |q| * |r|, largest first, and cut into launches of at most
// EXACT_LAUNCH_CELLS cells -- or of one pair per wave of the device, if that is more --, so that no single kernel holds the device for long
// ("Exact scores"). Every launch is persistent: 16 waves per CU at most, one pair per wave at a time.
static_assert(sizeof(BaExact) == sizeof(ba::Exact) && offsetof(BaExact, reference_idx) == offsetof(ba::Exact, reference_idx) &&
              offsetof(BaExact, rows) == offsetof(ba::Exact, rows), "BaExact and ba::Exact differ");
constexpr uint64_t EXACT_LAUNCH_CELLS = 1ull << 36;
constexpr uint32_t EXACT_WAVES_PER_CU = 16;
static_assert(ba::EXACT_TRACE_MAX_CELLS == BA_EXACT_TRACE_MAX_CELLS, "BA_EXACT_TRACE_MAX_CELLS and ba::EXACT_TRACE_MAX_CELLS differ");
// The length guards. Every pair must fit int32 scores; a profile column adds three int8 terms. traced: every pair must also fit a trace
// region; the profile sweep owns row 0, so a pair has |q| + 1 traced rows there.
static int exact_check_lengths(bool profile, bool traced, const uint32_t* ql, const uint32_t* rl, size_t n, const uint32_t* name) {
    const uint64_t max_len2 = profile ? ba::EXACT_MAX_LEN2_PROFILE : ba::EXACT_MAX_LEN2;
    for (size_t p = 0; p < n; p++)
        if ((uint64_t)ql[p] + rl[p] > max_len2)
            return fail(profile ? "exact: pair %zu (|q| = %u, profile length = %u) is too long for int32 scores: |q| + |r| may be %llu at most for a profile batch"
                                : "exact: pair %zu (|q| = %u, |r| = %u) is too long for int32 scores: |q| + |r| may be %llu at most",
                        name ? (size_t)name[p] : p, ql[p], rl[p], (unsigned long long)max_len2);
    for (size_t p = 0; traced && p < n; p++)
        if (((uint64_t)ql[p] + (profile ? 1 : 0)) * rl[p] > ba::EXACT_TRACE_MAX_CELLS)
            return fail(profile ? "exact: pair %zu (|q| = %u, profile length = %u) is too large for a traced matrix: (|q| + 1) * |r| may be %llu at most (BA_EXACT_TRACE_MAX_CELLS)"
                                : "exact: pair %zu (|q| = %u, |r| = %u) is too large for a traced matrix: |q| * |r| may be %llu at most (BA_EXACT_TRACE_MAX_CELLS)",
                        name ? (size_t)name[p] : p, ql[p], rl[p], (unsigned long long)ba::EXACT_TRACE_MAX_CELLS);
    return 0;
}
static_assert(sizeof(BaExactPath) == sizeof(ba::ExactPath) && offsetof(BaExactPath, r_end) == offsetof(ba::ExactPath, r_end), "BaExactPath and ba::ExactPath differ");
static_assert(ba::EXACT_OWN_MODE == BA_EXACT_OWN_MODE, "BA_EXACT_OWN_MODE and ba::EXACT_OWN_MODE differ");
// the batch's own mode asks for another sweep than k_exact's: the flag is set and the batch is not a plain sequence batch
static bool exact_own_sweep(const BaBatch* b, uint32_t what) {
    return (what & BA_EXACT_OWN_MODE) && (b->kind == BA_KIND_PROFILE_ || special_of(b->mode));
}
// paths: the call returns optimal paths too (ba_*_exact_cigars)
static int exact_refusals(const BaBatch* b, uint32_t what, const void* out, bool paths = false) {
    if (!out) return fail("null argument: out");
    const uint32_t quantity = what & ~(uint32_t)BA_EXACT_OWN_MODE;
    if (quantity != BA_EXACT_GLOBAL && quantity != BA_EXACT_EXTEND) return fail("exact: unknown quantity %u (BA_EXACT_GLOBAL or BA_EXACT_EXTEND)", what);
    if (!(what & BA_EXACT_OWN_MODE)) {
        if (b->kind == BA_KIND_PROFILE_) return fail("exact: profile batches are not supported (position-specific gap costs)");
        if (special_of(b->mode)) return fail("exact: batches with BA_LOCAL_START or BA_FREE_QUERY_* are not supported");
    } else {
        if (b->kind == BA_KIND_PROFILE_ && special_of(b->mode))
            return fail("exact: BA_EXACT_OWN_MODE does not cover a profile batch with BA_LOCAL_START or BA_FREE_QUERY_* (that combination has no definition yet)");
        if (paths && exact_own_sweep(b, what))
            return fail("exact: BA_EXACT_OWN_MODE gives scores only: no paths for a profile batch or a batch with BA_LOCAL_START or BA_FREE_QUERY_* (ba_*_exact)");
    }
    if (b->handle_mode) return fail("exact: not a batch");
    if (b->in_flight) return fail("exact: the batch has a launch in flight (ba_batch_wait first)");
    if (!b->n) return fail("exact: the batch holds no pairs (a reload failed)");
    return 0;
}
// form: scores only; the paths too (ba_batch_exact_cigars) -- the record's runs are left on the device in b->xt_runs at the offsets of
// b->xt_off; or the paths in the batch's own mode (ba_batch_exact_paths), whatever the batch: the traced own-mode kernels of ba_exact.hip, which
// also leave the start cells in b->xt_start
enum { EXACT_FORM_SCORES = 0, EXACT_FORM_CIGARS = 1, EXACT_FORM_PATHS = 2 };
static int batch_exact_device(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* devpos, size_t m, BaExact* out, int form = EXACT_FORM_SCORES) {
    const bool traced = form != EXACT_FORM_SCORES, paths = form == EXACT_FORM_PATHS;
    if (paths) what |= BA_EXACT_OWN_MODE;
    if (exact_refusals(b, what, out, form == EXACT_FORM_CIGARS)) return 1;
    const bool profile = b->kind == BA_KIND_PROFILE_, own = paths || exact_own_sweep(b, what);   // (on a plain sequence batch the flag changes nothing)
    what &= ~(uint32_t)BA_EXACT_OWN_MODE;
    float& ms_out = paths ? b->xp_ms : traced ? b->xt_ms : b->exact_ms;
    uint64_t& cells_out = paths ? b->xp_cells : traced ? b->xt_cells : b->exact_cells;
    ms_out = 0; cells_out = 0;
    if (!m) return 0;
    if (m > 0x7fffffffu) return fail("exact: too many records in one request");
    HIP_TRY(hipSetDevice(b->device));
    std::vector<uint32_t> ql(b->n), rl(b->n);
    HIP_TRY(hipMemcpy(ql.data(), b->q_len.p, (size_t)b->n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rl.data(), b->r_len.p, (size_t)b->n * 4, hipMemcpyDeviceToHost));
    if (exact_check_lengths(profile, false, ql.data(), rl.data(), b->n, b->h_order.empty() ? nullptr : b->h_order.data())) return 1;
    if (traced)   // (the requested pairs only: the others need no region)
        for (size_t k = 0; k < m; k++) {
            const uint32_t d = devpos[k];
            if (d == ba::EXACT_NO_PAIR) continue;
            const uint32_t* name = b->h_order.empty() ? &d : &b->h_order[d];
            if (exact_check_lengths(profile, true, &ql[d], &rl[d], 1, name)) return 1;
        }
    // (the profile sweep shares this cost model: it also walks row 0, one row in |q| + 1, which neither the order nor the cuts notice)
    auto cost = [&](uint32_t k) { const uint32_t d = devpos[k]; return d == ba::EXACT_NO_PAIR ? 0ull : (uint64_t)ql[d] * rl[d]; };
    std::vector<uint32_t> rec(m);
    for (size_t k = 0; k < m; k++) rec[k] = (uint32_t)k;
    std::stable_sort(rec.begin(), rec.end(), [&](uint32_t a, uint32_t c) { return cost(a) > cost(c); });
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    const uint32_t max_wgs = (uint32_t)std::max(1, cus) * EXACT_WAVES_PER_CU / ba::EXACT_WAVES;
    std::vector<uint32_t> work(2 * m), first{0};   // first: the launches' first records
    uint32_t max_r = 0;
    uint64_t cells = 0;
    for (size_t s = 0; s < m; s++) {
        const uint32_t d = devpos[rec[s]];
        work[2 * s] = d; work[2 * s + 1] = rec[s];
        if (d == ba::EXACT_NO_PAIR) continue;
        max_r = std::max(max_r, rl[d]);
        const uint64_t c = ((uint64_t)ql[d] + 1) * ((uint64_t)rl[d] + 1);
        // (a launch is cut only once every wave of the device has a pair: long pairs would otherwise leave most of it idle)
        if (cells + c > EXACT_LAUNCH_CELLS && s - first.back() >= (size_t)max_wgs * ba::EXACT_WAVES) { first.push_back((uint32_t)s); cells = 0; }
        cells += c;
    }
    first.push_back((uint32_t)m);
    const size_t launches = first.size() - 1;
    uint32_t wgs = (uint32_t)std::min<uint64_t>(max_wgs, (std::min<uint64_t>(m, first[1]) + ba::EXACT_WAVES - 1) / ba::EXACT_WAVES);   // (the first launch is the largest)
    uint32_t tr_waves = 0;
    uint64_t tr_stride = 0;
    std::vector<uint64_t> rev_off;
    if (traced) {
        // every record's reversed runs (|q| + |r| at most), the counts and the offsets first; the trace regions take what is left
        rev_off.resize(m + 1);
        rev_off[0] = 0;
        for (size_t k = 0; k < m; k++) {
            const uint32_t d = devpos[k];
            rev_off[k + 1] = rev_off[k] + (d == ba::EXACT_NO_PAIR ? 0ull : (uint64_t)ql[d] + rl[d]);
            if (d != ba::EXACT_NO_PAIR) tr_stride = std::max(tr_stride, ba::exact_trace_stride(ql[d] + (profile ? 1u : 0u), rl[d]));   // (row 0 of a profile is swept)
        }
        tr_stride = std::max<uint64_t>(tr_stride, 64);
        const uint64_t rev_bytes = std::max<uint64_t>(rev_off[m], 1) * 4;
        if (b->xt_rev.bytes < rev_bytes) {
            size_t free_b = 0, total_b = 0;
            mem_info(&free_b, &total_b);
            if (rev_bytes > free_b + b->xt_rev.bytes)
                return fail("exact: the runs of the request need %llu bytes of device memory before they are merged (4 x the sum of |q| + |r|), %zu are free",
                            (unsigned long long)rev_bytes, free_b + b->xt_rev.bytes);
            if (b->xt_rev.alloc(rev_bytes)) return 1;
        }
        if (b->xt_rev_off.bytes < (m + 1) * 8 && b->xt_rev_off.alloc((m + 1) * 8)) return 1;
        if (b->xt_nrun.bytes < m * 4 && b->xt_nrun.alloc(m * 4)) return 1;
        if (b->xt_off.bytes < (m + 1) * 8 && b->xt_off.alloc((m + 1) * 8)) return 1;
        if (paths && b->xt_start.bytes < m * 8 && b->xt_start.alloc(m * 8)) return 1;
        // as many concurrent waves as free memory holds regions of the largest pair (a sixteenth is left for the run array), one at least
        const uint64_t region = tr_stride * 4;
        uint32_t want = wgs * ba::EXACT_WAVES;
        if (b->xt_trace.bytes < want * region) {
            size_t free_b = 0, total_b = 0;
            mem_info(&free_b, &total_b);
            const uint64_t avail = (uint64_t)free_b + b->xt_trace.bytes;
            const uint64_t fit = (avail - avail / 16) / region;
            if (!fit)
                return fail("exact: one trace region needs %llu bytes of device memory (the request's largest pair at 4 bits per cell), %llu are free",
                            (unsigned long long)region, (unsigned long long)avail);
            want = (uint32_t)std::min<uint64_t>(want, fit);
            if (want >= ba::EXACT_WAVES) want -= want % ba::EXACT_WAVES;
            if (b->xt_trace.bytes < want * region && b->xt_trace.alloc(want * region)) return 1;
        }
        tr_waves = want;
        wgs = (tr_waves + ba::EXACT_WAVES - 1) / ba::EXACT_WAVES;
    }
    const uint64_t stride = ba::exact_row_stride(max_r), row_bytes = (uint64_t)wgs * ba::EXACT_WAVES * stride * 8;
    if (b->ex_rows.bytes < row_bytes) {
        size_t free_b = 0, total_b = 0;
        mem_info(&free_b, &total_b);
        if (row_bytes > free_b + b->ex_rows.bytes)
            return fail("exact: the row buffers need %llu bytes of device memory (%u waves x %llu reference columns x 8), %zu are free", (unsigned long long)row_bytes,
                        wgs * ba::EXACT_WAVES, (unsigned long long)stride, free_b + b->ex_rows.bytes);
        if (b->ex_rows.alloc(row_bytes)) return 1;
    }
    if (b->ex_work.bytes < 2 * m * 4 && b->ex_work.alloc(2 * m * 4)) return 1;
    if (b->ex_out.bytes < m * sizeof(ba::Exact) && b->ex_out.alloc(m * sizeof(ba::Exact))) return 1;
    if (b->ex_counter.bytes < launches * 4 && b->ex_counter.alloc(launches * 4)) return 1;
    HIP_TRY(hipMemcpy(b->ex_work.p, work.data(), 2 * m * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(b->ex_counter.p, 0, launches * 4, b->stream));
    if (!b->ev_x0) HIP_TRY(hipEventCreate(&b->ev_x0));
    if (!b->ev_x1) HIP_TRY(hipEventCreate(&b->ev_x1));
    ba::ExactParams xp{};
    xp.what = what; xp.x_drop = x_drop; xp.kind = own ? b->kind : seq_kind(b->kind); xp.gap_open = b->gap_open; xp.gap_extend = b->gap_extend;
    xp.matrix = b->matrix.as<int8_t>(); xp.matrix_bytes = (uint32_t)std::min<size_t>(b->matrix.bytes, 1024);
    xp.pool = b->pool.as<uint8_t>(); xp.q_off = b->q_off.as<uint64_t>(); xp.q_len = b->q_len.as<uint32_t>();
    xp.r_off = b->r_off.as<uint64_t>(); xp.r_len = b->r_len.as<uint32_t>();
    xp.rows = b->ex_rows.as<int32_t>(); xp.row_stride = stride; xp.out = b->ex_out.as<ba::Exact>();
    if (traced) {
        HIP_TRY(hipMemcpy(b->xt_rev_off.p, rev_off.data(), (m + 1) * 8, hipMemcpyHostToDevice));
        xp.trace = b->xt_trace.as<uint32_t>(); xp.trace_stride = tr_stride;
        xp.rev = b->xt_rev.as<uint32_t>(); xp.rev_off = b->xt_rev_off.as<uint64_t>(); xp.nrun = b->xt_nrun.as<uint32_t>();
        xp.eq = (b->mode & BA_CIGAR_EQ) ? 1u : 0u;
    }
    HIP_TRY(hipEventRecord(b->ev_x0, b->stream));
    for (size_t l = 0; l < launches; l++) {
        xp.n = first[l + 1] - first[l];
        xp.work = b->ex_work.as<uint32_t>() + 2 * (size_t)first[l];
        xp.counter = b->ex_counter.as<uint32_t>() + l;
        uint32_t waves = std::min<uint32_t>(tr_waves, xp.n);   // (the traced forms)
        if (waves >= ba::EXACT_WAVES) waves -= waves % ba::EXACT_WAVES;
        if (traced && !paths) {
            HIP_TRY(ba_launch_exact_trace(b->stream, &xp, waves));
        } else if (own) {   // k_exact_mode / k_exact_profile: the same records, row buffers (two words per column) and launch geometry
            ba::ExactModeParams mp{};
            mp.x = xp;
            mp.start = (b->mode & BA_LOCAL_START) ? ba::EXACT_START_LOCAL : (b->mode & BA_FREE_QUERY_START_GAPS) ? ba::EXACT_START_FREE_ROW0 : ba::EXACT_START_GLOBAL;
            mp.end_free = (b->mode & BA_FREE_QUERY_END_GAPS) ? 1u : 0u;
            mp.max_size = (uint32_t)b->max_size;
            if (paths) HIP_TRY(ba_launch_exact_modes_trace(b->stream, &mp, b->xt_start.as<uint32_t>(), waves));
            else HIP_TRY(ba_launch_exact_modes(b->stream, &mp, std::min<uint32_t>(wgs, (xp.n + ba::EXACT_WAVES - 1) / ba::EXACT_WAVES)));
        } else
            HIP_TRY(ba_launch_exact(b->stream, &xp, std::min<uint32_t>(wgs, (xp.n + ba::EXACT_WAVES - 1) / ba::EXACT_WAVES)));
    }
    if (traced) {   // sizes -> offsets -> one run array, in record order
        HIP_TRY(ba_launch_offsets(b->stream, b->xt_nrun.as<uint32_t>(), b->xt_off.as<uint64_t>(), (uint32_t)m));
        uint64_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, b->xt_off.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (b->xt_runs.bytes < total * 4 && b->xt_runs.alloc(total * 4)) return 1;
        HIP_TRY(ba_launch_exact_runs(b->stream, b->xt_rev.as<uint32_t>(), b->xt_rev_off.as<uint64_t>(), b->xt_nrun.as<uint32_t>(), b->xt_off.as<uint64_t>(),
                                     b->xt_runs.as<uint32_t>(), (uint32_t)m));
    }
    HIP_TRY(hipEventRecord(b->ev_x1, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipEventElapsedTime(&ms_out, b->ev_x0, b->ev_x1));
    HIP_TRY(hipMemcpy(out, b->ex_out.p, m * sizeof(ba::Exact), hipMemcpyDeviceToHost));
    cells = 0;
    for (size_t k = 0; k < m; k++) if (devpos[k] != ba::EXACT_NO_PAIR) cells += (uint64_t)out[k].rows * ((uint64_t)rl[devpos[k]] + 1);
    cells_out = cells;
    return 0;
}
// `which` (null: every pair) in the caller's order -> device positions
static int exact_devpos(const BaBatch* b, const uint32_t* which, size_t n_which, std::vector<uint32_t>& devpos) {
    const size_t m = which ? n_which : b->n;
    std::vector<uint32_t> dev_of;
    devpos.resize(m);
    if (!b->h_order.empty()) { dev_of.resize(b->n); for (uint32_t s = 0; s < b->n; s++) dev_of[b->h_order[s]] = s; }
    for (size_t k = 0; k < m; k++) {
        const uint32_t p = which ? which[k] : (uint32_t)k;
        if (p >= b->n) return fail("exact: which[%zu] = %u is out of range (the batch holds %u pairs)", k, p, b->n);
        devpos[k] = dev_of.empty() ? p : dev_of[p];
    }
    return 0;
}
static int batch_exact(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* which, size_t n_which, BaExact* out) {
    if (!b) return fail("null batch");
    if (exact_refusals(b, what, out)) return 1;
    std::vector<uint32_t> devpos;
    if (exact_devpos(b, which, n_which, devpos)) return 1;
    return batch_exact_device(b, what, x_drop, devpos.data(), devpos.size(), out);
}
// The records, the run offsets (records + 1) and, with `runs`, the runs. A request equal to the last one on the same pairs is answered from
// what that one left on the device.
// Rec = BaExact: ba_batch_exact_cigars. Rec = BaExactPath: ba_batch_exact_paths -- the matrix of the batch's own mode, with the start cells.
template <class Rec>
static int batch_exact_cigars(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* which, size_t n_which, Rec* out, uint64_t* run_off, uint32_t* runs,
                              uint64_t capacity) {
    constexpr int form = std::is_same<Rec, BaExact>::value ? EXACT_FORM_CIGARS : EXACT_FORM_PATHS;
    if (!b) return fail("null batch");
    if (!out) return fail("null argument: out");
    if (!run_off) return fail("null argument: run_off");
    if (form == EXACT_FORM_PATHS) what |= BA_EXACT_OWN_MODE;   // (the flag may be given and changes nothing)
    if (exact_refusals(b, what, out, form == EXACT_FORM_CIGARS)) return 1;
    std::vector<uint32_t> devpos;
    if (exact_devpos(b, which, n_which, devpos)) return 1;
    const size_t m = devpos.size();
    const bool kept = b->xt_valid && b->xt_form == form && b->xt_what == what && b->xt_x_drop == x_drop && b->xt_loads == b->loads && b->xt_devpos == devpos;
    if (!kept) {
        b->xt_valid = false;
        b->xt_out.assign(m, BaExact{}); b->xt_h_off.assign(m + 1, 0); b->xt_h_start.assign(2 * m, 0);
        if (batch_exact_device(b, what, x_drop, devpos.data(), m, b->xt_out.data(), form)) return 1;
        if (m) HIP_TRY(hipMemcpy(b->xt_h_off.data(), b->xt_off.p, (m + 1) * 8, hipMemcpyDeviceToHost));
        if (m && form == EXACT_FORM_PATHS) HIP_TRY(hipMemcpy(b->xt_h_start.data(), b->xt_start.p, m * 8, hipMemcpyDeviceToHost));
        b->xt_form = form; b->xt_what = what; b->xt_x_drop = x_drop; b->xt_loads = b->loads; b->xt_devpos = devpos; b->xt_valid = true;
    } else HIP_TRY(hipSetDevice(b->device));
    if constexpr (std::is_same<Rec, BaExact>::value) std::copy(b->xt_out.begin(), b->xt_out.end(), out);
    else
        for (size_t k = 0; k < m; k++) {
            const BaExact& x = b->xt_out[k];
            out[k] = BaExactPath{x.score, b->xt_h_start[2 * k], b->xt_h_start[2 * k + 1], x.query_idx, x.reference_idx, x.rows};
        }
    std::copy(b->xt_h_off.begin(), b->xt_h_off.end(), run_off);
    if (!runs) return 0;
    const uint64_t total = b->xt_h_off[m];
    if (capacity < total) return fail("exact: the runs buffer holds %llu runs, the request has %llu", (unsigned long long)capacity, (unsigned long long)total);
    if (total) HIP_TRY(hipMemcpy(runs, b->xt_runs.p, total * 4, hipMemcpyDeviceToHost));
    return 0;
}
static int extend_exact(BaExtendBatch* e, int32_t x_drop, const uint32_t* which, size_t n_which, BaExact* left, BaExact* right, int32_t* score) {
    if (!e) return fail("null batch");
    if (!left || !right || !score) return fail("null argument");
    if (!e->n) return fail("exact: the batch holds no seeds (a reload failed)");
    const size_t m = which ? n_which : e->n;
    if (!m) return 0;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> side(2 * (size_t)e->n), sel(m), devpos(2 * m);
    HIP_TRY(hipMemcpy(side.data(), e->side.p, side.size() * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < m; k++) {
        const uint32_t s = which ? which[k] : (uint32_t)k;
        if (s >= e->n) return fail("exact: which[%zu] = %u is out of range (the batch holds %u seeds)", k, s, e->n);
        sel[k] = s; devpos[2 * k] = side[2 * (size_t)s]; devpos[2 * k + 1] = side[2 * (size_t)s + 1];
    }
    std::vector<BaExact> rec(2 * m, BaExact{});
    if (e->inner && e->n_sides && batch_exact_device(e->inner.get(), BA_EXACT_EXTEND, x_drop, devpos.data(), 2 * m, rec.data())) return 1;
    DevBuf d_sel, d_seed;
    if (d_sel.alloc(m * 4) || d_seed.alloc(m * 4)) return 1;
    HIP_TRY(hipMemcpy(d_sel.p, sel.data(), m * 4, hipMemcpyHostToDevice));
    const ba::ExtendParams ep = e->params();
    HIP_TRY(ba_launch_exact_seed(e->stream, &ep, d_sel.as<uint32_t>(), (uint32_t)m, d_seed.as<int32_t>()));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(score, d_seed.p, m * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < m; k++) { left[k] = rec[2 * k]; right[k] = rec[2 * k + 1]; score[k] += rec[2 * k].score + rec[2 * k + 1].score; }
    return 0;
}
// The optimal path of every requested seed: both sides' EXTEND paths from the traced k_exact over the inner batch (record 2k the left side,
// over the reversed prefixes, 2k + 1 the right one; their runs stay on the device), joined with the seed's ungapped columns by k_exact_join
// -- counts, offsets, runs. The records are in the coordinates of ba_extend_batch_results.
static int extend_exact_paths(BaExtendBatch* e, int32_t x_drop, const uint32_t* which, size_t n_which, BaExactPath* out, BaExact* left, BaExact* right,
                              uint64_t* run_off, uint32_t* runs, uint64_t capacity) {
    if (!e) return fail("null batch");
    if (!out) return fail("null argument: out");
    if (!run_off) return fail("null argument: run_off");
    if (!e->n) return fail("exact: the batch holds no seeds (a reload failed)");
    const size_t m = which ? n_which : e->n;
    if (m > 0x3fffffffu) return fail("exact: too many records in one request");
    std::vector<uint32_t> sel(m);
    for (size_t k = 0; k < m; k++) {
        sel[k] = which ? which[k] : (uint32_t)k;
        if (sel[k] >= e->n) return fail("exact: which[%zu] = %u is out of range (the batch holds %u seeds)", k, sel[k], e->n);
    }
    HIP_TRY(hipSetDevice(e->device));
    const bool kept = e->xp_valid && e->xp_x_drop == x_drop && e->xp_which == sel;
    if (!kept) {
        e->xp_valid = false;
        e->xp_out.assign(m, BaExactPath{}); e->xp_left.assign(m, BaExact{}); e->xp_right.assign(m, BaExact{}); e->xp_h_off.assign(m + 1, 0);
        if (m) {
            std::vector<uint32_t> side(2 * (size_t)e->n), devpos(2 * m), q_seed(e->n), r_seed(e->n), seed_len(e->n);
            HIP_TRY(hipMemcpy(side.data(), e->side.p, side.size() * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(q_seed.data(), e->q_seed.p, (size_t)e->n * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(r_seed.data(), e->r_seed.p, (size_t)e->n * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(seed_len.data(), e->seed_len.p, (size_t)e->n * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < m; k++) { devpos[2 * k] = side[2 * (size_t)sel[k]]; devpos[2 * k + 1] = side[2 * (size_t)sel[k] + 1]; }
            std::vector<BaExact> rec(2 * m, BaExact{});
            const bool sides = e->inner && e->n_sides;
            if (sides) {
                e->inner->xt_valid = false;   // (the inner batch's buffers now hold this request)
                if (batch_exact_device(e->inner.get(), BA_EXACT_EXTEND, x_drop, devpos.data(), 2 * m, rec.data(), EXACT_FORM_CIGARS)) return 1;
            } else {   // every side's run range is empty
                if (e->xp_no_off.bytes < (2 * m + 1) * 8 && e->xp_no_off.alloc((2 * m + 1) * 8)) return 1;
                HIP_TRY(hipMemset(e->xp_no_off.p, 0, (2 * m + 1) * 8));
            }
            if (e->xp_seed.bytes < m * 4 && e->xp_seed.alloc(m * 4)) return 1;
            if (e->xp_sel.bytes < m * 4 && e->xp_sel.alloc(m * 4)) return 1;
            if (e->xp_nrun.bytes < m * 4 && e->xp_nrun.alloc(m * 4)) return 1;
            if (e->xp_off.bytes < (m + 1) * 8 && e->xp_off.alloc((m + 1) * 8)) return 1;
            HIP_TRY(hipMemcpy(e->xp_sel.p, sel.data(), m * 4, hipMemcpyHostToDevice));
            const ba::ExtendParams ep = e->params();
            HIP_TRY(ba_launch_exact_seed(e->stream, &ep, e->xp_sel.as<uint32_t>(), (uint32_t)m, e->xp_seed.as<int32_t>()));
            ba::ExactJoinParams jp{};
            jp.m = (uint32_t)m; jp.eq = (e->mode & BA_CIGAR_EQ) ? 1u : 0u; jp.sel = e->xp_sel.as<uint32_t>();
            jp.seed_len = ep.seed_len; jp.seed_pool = ep.seed_pool; jp.seed_q = ep.seed_q; jp.seed_r = ep.seed_r;
            jp.side_runs = sides ? e->inner->xt_runs.as<uint32_t>() : nullptr;
            jp.side_off = sides ? e->inner->xt_off.as<uint64_t>() : e->xp_no_off.as<uint64_t>();
            jp.nrun = e->xp_nrun.as<uint32_t>(); jp.off = e->xp_off.as<uint64_t>(); jp.runs = nullptr;
            HIP_TRY(ba_launch_exact_join(e->stream, &jp));
            HIP_TRY(ba_launch_offsets(e->stream, e->xp_nrun.as<uint32_t>(), e->xp_off.as<uint64_t>(), (uint32_t)m));
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipMemcpy(e->xp_h_off.data(), e->xp_off.p, (m + 1) * 8, hipMemcpyDeviceToHost));
            const uint64_t total = e->xp_h_off[m];
            if (e->xp_runs.bytes < total * 4 && e->xp_runs.alloc(total * 4)) return 1;
            jp.runs = e->xp_runs.as<uint32_t>();
            HIP_TRY(ba_launch_exact_join(e->stream, &jp));
            HIP_TRY(hipStreamSynchronize(e->stream));
            std::vector<int32_t> seed_score(m);
            HIP_TRY(hipMemcpy(seed_score.data(), e->xp_seed.p, m * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < m; k++) {
                const BaExact &l = rec[2 * k], &r = rec[2 * k + 1];
                const uint32_t s = sel[k];
                e->xp_left[k] = l; e->xp_right[k] = r;
                e->xp_out[k] = BaExactPath{l.score + seed_score[k] + r.score, q_seed[s] - l.query_idx, r_seed[s] - l.reference_idx,
                                           q_seed[s] + seed_len[s] + r.query_idx, r_seed[s] + seed_len[s] + r.reference_idx, l.rows + r.rows};
            }
        }
        e->xp_x_drop = x_drop; e->xp_which = sel; e->xp_valid = true;
    }
    std::copy(e->xp_out.begin(), e->xp_out.end(), out);
    if (left) std::copy(e->xp_left.begin(), e->xp_left.end(), left);
    if (right) std::copy(e->xp_right.begin(), e->xp_right.end(), right);
    std::copy(e->xp_h_off.begin(), e->xp_h_off.end(), run_off);
    if (!runs) return 0;
    const uint64_t total = e->xp_h_off[m];
    if (capacity < total) return fail("exact: the runs buffer holds %llu runs, the request has %llu", (unsigned long long)capacity, (unsigned long long)total);
    if (total) HIP_TRY(hipMemcpy(runs, e->xp_runs.p, total * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ alignment strings (ba_*_text)
// The format and flags of `what`, against the batch's kind and mode (the other refusals are the stats calls').
static int text_check(int kind, uint32_t mode, uint32_t what) {
    const uint32_t fmt = what & ba::TEXT_FORMAT;
    if ((what & ~(ba::TEXT_FORMAT | ba::TEXT_SOFT_CLIP)) || fmt > ba::TEXT_CS)
        return fail("text: unknown what 0x%x (BA_TEXT_CIGAR, BA_TEXT_MD or BA_TEXT_CS; BA_TEXT_CIGAR | BA_TEXT_SOFT_CLIP)", what);
    if ((what & ba::TEXT_SOFT_CLIP) && fmt != ba::TEXT_CIGAR) return fail("text: BA_TEXT_SOFT_CLIP goes with BA_TEXT_CIGAR only");
    if (!(mode & BA_TRACE)) return fail("text: the batch was created without BA_TRACE (the strings are rendered from the CIGAR runs)");
    if (fmt != ba::TEXT_CIGAR && kind == BA_KIND_PROFILE_) return fail("text: MD and cs need reference letters, and a profile batch has none (BA_TEXT_CIGAR only)");
    if (fmt != ba::TEXT_CIGAR && kind == BA_KIND_BYTES)
        return fail("text: MD and cs are letter formats, and a ByteMatrix batch compares raw bytes (BA_TEXT_CIGAR only)");
    return 0;
}
// Size (k_text_len + k_text_offsets, unless the sizes of this run and format are on the device already) and, with `text`, render
// (k_text_write) the n pairs described by tp; offsets (n + 1) and the text are copied to the host.
static int text_kernels(TextState& T, int device, hipStream_t stream, uint64_t run, ba::TextParams tp, uint64_t cap_n, const std::vector<uint32_t>* order,
                        uint64_t* offsets, char* text, uint64_t capacity) {
    HIP_TRY(hipSetDevice(device));
    if ((!T.len.p || !T.off.p) && (T.len.alloc(cap_n * 4) || T.off.alloc((cap_n + 1) * 8))) return 1;
    for (hipEvent_t& e : T.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    const uint32_t n = tp.n;
    if (order && !order->empty()) {
        if (!T.pos.p && T.pos.alloc(cap_n * 4)) return 1;
        tp.out_pos = T.pos.as<uint32_t>();
    }
    tp.len = T.len.as<uint32_t>(); tp.offsets = T.off.as<uint64_t>();
    T.ms = 0;
    float ms = 0;
    if (!(T.sized && T.run == run && T.what == tp.what)) {
        T.sized = false;
        if (tp.out_pos) HIP_TRY(hipMemcpy(T.pos.p, order->data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipEventRecord(T.ev[0], stream));
        HIP_TRY(ba_launch_text_len(stream, &tp));
        HIP_TRY(hipEventRecord(T.ev[1], stream));
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
        T.ms += ms;
        T.sized = true; T.run = run; T.what = tp.what;
    }
    HIP_TRY(hipMemcpy(offsets, T.off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    if (!text) return 0;
    const uint64_t total = offsets[n];
    if (capacity < total)
        return fail("text buffer too small: the text needs %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)capacity);
    if (!total) return 0;
    if (total > T.buf_cap) {
        if (T.buf.alloc(total)) { T.buf_cap = 0; return 1; }
        T.buf_cap = total;
    }
    tp.text = T.buf.as<char>();
    HIP_TRY(hipEventRecord(T.ev[0], stream));
    HIP_TRY(ba_launch_text_write(stream, &tp));
    HIP_TRY(hipEventRecord(T.ev[1], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
    T.ms += ms;
    HIP_TRY(hipMemcpy(text, T.buf.p, total, hipMemcpyDeviceToHost));
    return 0;
}
// One traced batch after its run, in the caller's pair order: the runs are the final ones (re-runs are merged by ba_batch_wait), the
// sequences the batch's images.
static int batch_text_device(BaBatch* b, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {
    if (text_check(b->kind, b->mode, what)) return 1;
    if (b->in_flight) return fail("text: the batch has a launch in flight (ba_batch_wait first)");
    if (!b->ran) return fail("text: the batch has not finished a run (ba_batch_run, or ba_batch_launch and ba_batch_wait)");
    ba::TextParams tp{};
    tp.n = b->n; tp.kind = seq_kind(b->kind); tp.what = what;
    tp.seq = b->pool.as<uint8_t>(); tp.skip = 1; tp.strand = nullptr;
    tp.q_off = b->q_off.as<uint64_t>(); tp.q_len = b->q_len.as<uint32_t>(); tp.r_off = b->r_off.as<uint64_t>(); tp.r_len = b->r_len.as<uint32_t>();
    tp.q_end = b->qidx.as<uint32_t>(); tp.r_end = b->ridx.as<uint32_t>(); tp.status = b->status.as<uint32_t>();
    tp.nrun = b->cig_len.as<uint32_t>(); tp.run_end = b->cig_off.as<uint64_t>(); tp.ops = b->cig_ops.as<uint32_t>();
    return text_kernels(b->text, b->device, b->stream, b->runs_done, tp, b->cap_n, &b->h_order, offsets, text, capacity);
}

// A spliced batch (ba_extend_batch_text, ba_chain_batch_text; run_call: the name of its run call): the spliced runs (caller's order,
// out_off / runs) from the unit's start; the oriented query and the reference read from the caller's bytes on the device (raw), by
// k_pack_images' rule. (The pieces' texts cannot be joined: the equal stretches merge across the seed or the anchors.)
static int spliced_text(Spliced* e, const char* run_call, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {
    if (!e) return fail("null batch");
    if (!offsets) return fail("null argument: offsets");
    if (text_check(e->kind, e->mode, what)) return 1;
    if (!e->ran) return fail("text: the batch has not finished a run (%s)", run_call);
    HIP_TRY(hipSetDevice(e->device));
    if (!e->t_strand.p && (e->t_raw_q.alloc(e->cap_n * 8) || e->t_raw_r.alloc(e->cap_n * 8) || e->t_ql.alloc(e->cap_n * 4) || e->t_rl.alloc(e->cap_n * 4) ||
                          e->t_strand.alloc(e->cap_n))) return 1;
    if (!e->t_uploaded) {
        if (h2d(e->t_raw_q, e->h_t_raw_q.data(), e->n) || h2d(e->t_raw_r, e->h_t_raw_r.data(), e->n) || h2d(e->t_ql, e->h_t_ql.data(), e->n) ||
            h2d(e->t_rl, e->h_t_rl.data(), e->n) || h2d(e->t_strand, e->h_t_strand.data(), e->n)) return 1;
        e->t_uploaded = true;
    }
    ba::TextParams tp{};
    tp.n = e->n; tp.kind = seq_kind(e->kind); tp.what = what;
    tp.seq = e->raw.as<uint8_t>(); tp.skip = 0; tp.strand = e->t_strand.as<uint8_t>();
    tp.q_off = e->t_raw_q.as<uint64_t>(); tp.q_len = e->t_ql.as<uint32_t>(); tp.r_off = e->t_raw_r.as<uint64_t>(); tp.r_len = e->t_rl.as<uint32_t>();
    tp.q_end = e->q_end.as<uint32_t>(); tp.r_end = e->r_end.as<uint32_t>(); tp.status = e->status.as<uint32_t>();
    tp.nrun = e->cigar_len.as<uint32_t>(); tp.run_end = e->out_off.as<uint64_t>(); tp.ops = e->runs.as<uint32_t>();
    return text_kernels(e->text, e->device, e->stream, e->runs_done, tp, e->cap_n, nullptr, offsets, text, capacity);
}

// ------------------------------------------------------------------ C ABI, Part 2
extern "C" {

const char* ba_last_error(void) { return g_err.c_str(); }
// Page-locked host memory for a caller's result buffers (CIGAR runs above all: 600 MB per 100 k 10 kbp pairs come back at 5 GB/s into
// pageable memory, at PCIe speed into this).
void* ba_host_alloc(uint64_t bytes) {
    if (ensure_device()) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 4, hipHostMallocDefault) != hipSuccess) { fail("hipHostMalloc(%llu bytes) failed", (unsigned long long)bytes); return nullptr; }
    return p;
}
void ba_host_free(void* p) { if (p) (void)hipHostFree(p); }
int ba_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int ba_set_device(int device) {
    int n = ba_device_count();
    if (device < 0 || device >= n) return fail("device %d out of range (%d devices)", device, n);
    g_device = device;
    HIP_TRY(hipSetDevice(device));
    return 0;
}
int ba_device_memory(uint64_t* free_bytes, uint64_t* total_bytes) {
    if (ensure_device()) return 1;
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}
uintptr_t block_percent_len(uintptr_t len, float p) {   // lib.rs:109-111
    size_t v = (size_t)std::round(p * (float)len);
    if (v < 32) v = 32;
    size_t pw = 1;
    while (pw < v) pw <<= 1;
    return pw < ((size_t)1 << 14) ? pw : ((size_t)1 << 14);
}

BaBatch* ba_batch_create(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                         const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n) {
    if (!matrix || !pool || !q_off || !q_len || !r_off || !r_len) { fail("null argument"); return nullptr; }
    if (kind == BA_KIND_PROFILE_) { fail("profile batches are created with ba_batch_create_profile"); return nullptr; }
    return batch_build(kind, matrix, gaps, size, x_drop, mode, n, false, [&](size_t p, int w, const uint8_t** ptr, size_t* len) {
        if (w == 0) { *ptr = pool + q_off[p]; *len = q_len[p]; } else { *ptr = pool + r_off[p]; *len = r_len[p]; }
    });
}
BaBatch* ba_batch_create_profile(const AAProfile* const* profiles, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                 const uint64_t* q_off, const uint32_t* q_len, uintptr_t n) {
    if (!profiles || !pool || !q_off || !q_len || n == 0 || !profiles[0]) { fail("null argument"); return nullptr; }
    const Gaps g{0, profiles[0]->gap_extend};   // the open costs are per position, inside the profiles
    return batch_build(BA_KIND_PROFILE_, nullptr, g, size, x_drop, mode, n, false,
                       [&](size_t p, int, const uint8_t** ptr, size_t* len) { *ptr = pool + q_off[p]; *len = q_len[p]; },
                       [&](size_t p) { return profiles[p]; });
}
int ba_batch_reload(BaBatch* b, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n) {
    if (!b || !pool || !q_off || !q_len || !r_off || !r_len) return fail("null argument");
    if (b->kind == BA_KIND_PROFILE_) return fail("profile batches are reloaded with ba_batch_reload_profile");
    return batch_reload(b, n, false, [&](size_t p, int w, const uint8_t** ptr, size_t* len) {
        if (w == 0) { *ptr = pool + q_off[p]; *len = q_len[p]; } else { *ptr = pool + r_off[p]; *len = r_len[p]; }
    });
}
int ba_batch_reload_profile(BaBatch* b, const AAProfile* const* profiles, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n) {
    if (!b || !profiles || !pool || !q_off || !q_len) return fail("null argument");
    if (b->kind != BA_KIND_PROFILE_) return fail("not a profile batch");
    return batch_reload(b, n, false, [&](size_t p, int, const uint8_t** ptr, size_t* len) { *ptr = pool + q_off[p]; *len = q_len[p]; },
                        [&](size_t p) { return profiles[p]; });
}
int ba_batch_run(BaBatch* b, float* kernel_ms) { return b ? batch_run(b, kernel_ms) : fail("null batch"); }
int ba_batch_launch(BaBatch* b) { return b ? batch_launch(b) : fail("null batch"); }
int ba_batch_wait(BaBatch* b, float* kernel_ms) { return b ? batch_wait(b, kernel_ms) : fail("null batch"); }
// What a run leaves on the device is read after its wait only. In flight -- between ba_batch_launch and a ba_batch_wait that succeeded, a wait that
// timed out included -- the kernels are still writing those buffers, and the batch's stream is non-blocking: a copy would not queue behind them. And a
// launch takes the last run's results away (batch_launch clears ran), so a wait that failed leaves none. Before any device call of a getter.
static int batch_results_refused(const BaBatch* b, const char* what) {
    if (b->in_flight) return fail("%s: the batch has a launch in flight (ba_batch_wait first)", what);
    if (!b->ran) return fail("ba_batch_run has not been called");
    return 0;
}
int ba_batch_results(BaBatch* b, int32_t* score, uint32_t* qi, uint32_t* ri, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    if (!b) return fail("null batch");
    if (batch_results_refused(b, "results")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    if (d2h(b->score, score, b->n) || d2h(b->qidx, qi, b->n) || d2h(b->ridx, ri, b->n) || d2h(b->cells, cells, b->n) ||
        d2h(b->cig_len, cigar_len, b->n) || d2h(b->status, status, b->n)) return 1;
    to_caller_order(b->h_order, score); to_caller_order(b->h_order, qi); to_caller_order(b->h_order, ri);
    to_caller_order(b->h_order, cells); to_caller_order(b->h_order, cigar_len); to_caller_order(b->h_order, status);
    return 0;
}
// Sum of width x height over the rectangles left on each pair's trace stack (Trace::blocks(), scan_block.rs:1676-1691): what
// the reference's "DP fraction" counts (examples/uc_accuracy.rs:88-89). Rectangles popped by a checkpoint restore are not in it.
int ba_batch_surviving_cells(BaBatch* b, uint64_t* cells) {
    if (!b || !cells) return fail("null argument");
    if (!(b->mode & BA_TRACE)) return fail("batch was created without BA_TRACE");
    if (batch_results_refused(b, "surviving cells")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    std::vector<uint32_t> w(b->n);
    if (d2h(b->trace_words, w.data(), b->n)) return 1;
    const uint64_t per_word = (b->mode & BA_LOCAL_START) ? 2 : 1;   // LOCAL_START: a zero-mask word follows every trace word
    for (uint32_t s = 0; s < b->n; s++) cells[b->h_order.empty() ? s : b->h_order[s]] = (uint64_t)w[s] / per_word * 8;
    return 0;
}
// Enqueue, behind the launch in flight (call between ba_batch_launch and ba_batch_wait), the gather of every pair's CIGAR runs into one
// dense device buffer in the caller's pair order. ba_batch_cigars then only copies. Optional: without it ba_batch_cigars gathers on demand.
int ba_batch_compact_cigars(BaBatch* b, uint32_t* pinned_out, uint64_t pinned_capacity) {
    if (!b) return fail("null batch");
    if (!(b->mode & BA_TRACE)) return fail("batch was created without BA_TRACE");
    if (!b->in_flight) return fail("ba_batch_compact_cigars goes between ba_batch_launch and ba_batch_wait");
    if (b->adaptive && b->pipe) return 0;   // (pair-slot batches may re-run pairs after the wait: gather on demand)
    HIP_TRY(hipSetDevice(b->device));
    if (!b->compact_off.p && b->compact_off.alloc((size_t)b->cap_n * 8)) return 1;
    if (!b->h_total) { HIP_TRY(hipHostMalloc((void**)&b->h_total, 64, hipHostMallocDefault)); }
    // pinned_out (memory from ba_host_alloc, which the device can write): the gather writes the runs straight into the caller's host
    // buffer -- over PCIe, inside the stream, right behind the kernels; ba_batch_cigars on the same pointer then has nothing left to copy
    // (a device-to-host copy issued while another batch's persistent launch fills the machine waits for that launch: copies of this size
    // are done by copy kernels). Otherwise: into a device buffer.
    uint32_t* out = pinned_out; uint64_t cap = pinned_capacity;
    if (out) {
        // a kernel writes through this pointer: it must be host memory the device can reach (ba_host_alloc / hipHostMalloc / hipHostRegister)
        // and hold pinned_capacity runs -- an ordinary malloc or numpy buffer here would be a GPU page fault that takes the process down
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, out) != hipSuccess) { (void)hipGetLastError(); return fail("ba_batch_compact_cigars: pinned_out is not page-locked host memory (use ba_host_alloc)"); }
        if (at.type != hipMemoryTypeHost) return fail("ba_batch_compact_cigars: pinned_out must be page-locked HOST memory (use ba_host_alloc)");
        void* base = nullptr; size_t range = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &range, (hipDeviceptr_t)at.devicePointer) == hipSuccess && base) {
            const size_t used = (size_t)((const char*)at.devicePointer - (const char*)base);
            if (range < used || (range - used) / 4 < cap) return fail("ba_batch_compact_cigars: pinned_out holds %zu runs, pinned_capacity says %llu", (range - used) / 4, (unsigned long long)cap);
        } else (void)hipGetLastError();
        out = (uint32_t*)at.devicePointer;   // (the address the device uses for this allocation; the same value for ba_host_alloc memory)
    }
    if (!out) {
        if (!b->compact.p) {
            // capacity: a third of the worst case (every cell of a pair's path its own run) covers any real alignment; if it ever does not,
            // the gather is skipped on the device and ba_batch_cigars falls back
            b->compact_cap = std::max<uint64_t>(b->cap_cig / 3, 1u << 20);
            if (b->compact.alloc(b->compact_cap * 4)) return 1;
        }
        out = b->compact.as<uint32_t>(); cap = b->compact_cap;
    }
    HIP_TRY(ba_launch_cigar_offsets_and_compact(b->stream, b->cig_ops.as<uint32_t>(), b->cig_off.as<uint64_t>(), b->cig_len.as<uint32_t>(),
                                                b->h_order.empty() ? nullptr : b->dev_of.as<uint32_t>(), b->compact_off.as<uint64_t>(), out,
                                                b->h_total, cap, b->n));
    b->compacted = true; b->compact_host = pinned_out; b->compact_used_cap = cap;
    return 0;
}
int ba_batch_cigars(BaBatch* b, uint32_t* runs, uint64_t capacity) {
    if (!b) return fail("null batch");
    if (!(b->mode & BA_TRACE)) return fail("batch was created without BA_TRACE");
    if (batch_results_refused(b, "cigars")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    if (b->compacted && b->retried == 0) {   // gathered behind the launch: one copy
        const unsigned long long total = *(volatile unsigned long long*)b->h_total;   // (written by the gather; the stream was synchronised by ba_batch_wait)
        if (total <= b->compact_used_cap) {
            if (total > capacity) return fail("cigar buffer too small: need %llu entries", total);
            if (b->compact_host) { if (runs != b->compact_host && total) memcpy(runs, b->compact_host, total * 4); }   // already in host memory
            else if (total) HIP_TRY(hipMemcpy(runs, b->compact.p, total * 4, hipMemcpyDeviceToHost));
            return 0;
        }
    }
    std::vector<uint32_t> len(b->n);
    if (d2h(b->cig_len, len.data(), b->n)) return 1;
    // runs go out pair after pair in the caller's order; the device arrays are in device order
    std::vector<uint64_t> out_off(b->n);
    uint64_t total = 0;
    if (b->h_order.empty()) for (uint32_t p = 0; p < b->n; p++) { out_off[p] = total; total += len[p]; }
    else {
        std::vector<uint32_t> dev_of(b->n);
        for (uint32_t s = 0; s < b->n; s++) dev_of[b->h_order[s]] = s;
        for (uint32_t p = 0; p < b->n; p++) { out_off[dev_of[p]] = total; total += len[dev_of[p]]; }
    }
    if (total > capacity) return fail("cigar buffer too small: need %llu entries", (unsigned long long)total);
    if (total == 0) return 0;
    DevBuf d_off, d_out;
    if (d_off.alloc(b->n * 8) || d_out.alloc(total * 4)) return 1;
    HIP_TRY(hipMemcpy(d_off.p, out_off.data(), b->n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ba_launch_compact_cigars(b->stream, b->cig_ops.as<uint32_t>(), b->cig_off.as<uint64_t>(), b->cig_len.as<uint32_t>(),
                                     d_off.as<uint64_t>(), d_out.as<uint32_t>(), b->n));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(runs, d_out.p, total * 4, hipMemcpyDeviceToHost));
    return 0;
}
#ifdef BA_DEV
// Development library only: the device-side known-answer test of the lane primitives (k_lane_kat, ba_kernels.hip). x: n_cells int16 values of
// D11_open, whole columns one after the other (form 0: 128 cells per column, four columns per wave; 1: 32 cells, sixteen per wave; 2 / 3 / 4: one
// column of 128 / 64 / 32 cells per wave; 5 / 6 / 7: k_multi's slots in the order of its loop of steps, four columns of 128 / two of 256 / one of 512 cells per wave);
// out: the columns' R11.
// (Beside it: ba_dev_lane_prim, the single helpers those scans are built from, and ba_dev_sort_keys, the seeding units' sort and search.)
int ba_dev_lane_scan(int form, const int16_t* x, uint32_t n_cells, int gap_extend, int16_t* out) {
    if (form < 0 || form > 7 || !x || !out) return fail("ba_dev_lane_scan: bad arguments");
    const uint32_t per_wave = (form <= 1 || form >= 5) ? 512u : (form == 2 ? 128u : (form == 3 ? 64u : 32u));
    if (n_cells == 0 || n_cells % per_wave) return fail("ba_dev_lane_scan: %u cells are not whole waves of %u", n_cells, per_wave);
    if (gap_extend > 0 || gap_extend < -128) return fail("ba_dev_lane_scan: gap_extend %d", gap_extend);
    DevBuf dx, dout;
    if (dx.alloc((size_t)n_cells * 2) || dout.alloc((size_t)n_cells * 2)) return 1;
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n_cells * 2, hipMemcpyHostToDevice));
    HIP_TRY(ba_launch_lane_kat(nullptr, form, dx.as<short>(), dout.as<short>(), gap_extend, n_cells / per_wave));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n_cells * 2, hipMemcpyDeviceToHost));
    return 0;
}
// ... of the single device helpers (k_prim_kat, ba_kernels.hip: op -> helper in its switch). x, out: four words per lane, whole waves of 64 lanes;
// a helper's operands are x[i] ^ (low word of k), k is also the op's wave-uniform operand (high word: multiplier, constant, parked value; all 64
// bits: a lane mask).
constexpr int BA_PRIM_OPS = 78;
int ba_dev_lane_prim(int op, const int32_t* x, uint32_t n_lanes, uint64_t k, int32_t* out) {
    if (op < 0 || op >= BA_PRIM_OPS || !x || !out) return fail("ba_dev_lane_prim: bad arguments");
    if (n_lanes == 0 || n_lanes % 64u) return fail("ba_dev_lane_prim: %u lanes are not whole waves of 64", n_lanes);
    const size_t bytes = (size_t)n_lanes * 16;
    DevBuf dx, dout;
    if (dx.alloc(bytes) || dout.alloc(bytes)) return 1;
    HIP_TRY(hipMemcpy(dx.p, x, bytes, hipMemcpyHostToDevice));
    HIP_TRY(ba_launch_prim_kat(nullptr, op, dx.as<int>(), dout.as<int>(), (unsigned long long)k, n_lanes / 64u));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
// ... and of ba::seed::sort_network<threads> and ba::seed::lower_bound (k_sort_kat): keys holds 2 n words. The first n are sorted in place in LDS by one
// workgroup of 64 (k_select_mark's) or 1024 (k_seeding_sort's, k_index_hit_sort's) threads, n within what those kernels sort in LDS; word n + i
// receives lower_bound of the caller's i-th key in the sorted array.
int ba_dev_sort_keys(int threads, uint64_t* keys, uint32_t n) {
    if ((threads != 64 && threads != 1024) || !keys) return fail("ba_dev_sort_keys: bad arguments");
    const uint32_t cap = threads == 64 ? ba::SELECT_MAX_PER_READ : ba::SEEDING_SORT_LDS;
    if (n > cap) return fail("ba_dev_sort_keys: %u keys, %d threads sort at most %u in LDS", n, threads, cap);
    if (n == 0) return 0;
    DevBuf dk, dlb;
    if (dk.alloc((size_t)n * 8) || dlb.alloc((size_t)n * 4)) return 1;
    HIP_TRY(hipMemcpy(dk.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ba_launch_sort_kat(nullptr, threads, dk.as<uint64_t>(), n, dlb.as<uint32_t>()));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> lb(n);
    HIP_TRY(hipMemcpy(keys, dk.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lb.data(), dlb.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) keys[n + i] = lb[i];
    return 0;
}
// ... and the kernel catalogue (tests/test_kernel_catalogue.py): the forms -- 0: there is no such kernel -- that the library holds of a family
// (ba::KernelFamily) for a matrix kind, a block class (0 .. 4: 128 << class cells, 5: row-tiled) and the plain / special modes. Launches nothing.
int ba_dev_kernel_forms(int family, int kind, int pclass, int special) {
    const ba::KernelEntry* k = find_kernel(family, kind, pclass, special);
    return !k ? 0 : (k->fn[1][0][0] ? 2 : 1);
}
#endif
int ba_batch_prof(BaBatch* b, uint64_t out[128]) {   // development: phase timers of a -DBA_TIMING build (all per-pair launches of a batch add up)
    if (!b) return fail("null batch");
    if (batch_results_refused(b, "timers")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpy(out, b->prof.p, 1024, hipMemcpyDeviceToHost));
    return 0;
}
int ba_batch_info(BaBatch* b, uint64_t out[4]) {
    if (!b) return fail("null batch");
    out[0] = (uint64_t)b->grid * b->wpw; out[1] = b->lds / b->wpw; out[2] = b->trace.bytes; out[3] = b->pool_bytes;
    return 0;
}
// Cells of the speculative, untraced rectangles of the last run (X-drop + TRACE batches: the chain of grows that closes an alignment,
// ba_driver.hpp run()): part of the computed cells, filled without trace flags and location bookkeeping (14 instead of 20 int16
// operations per cell). Pairs re-run for a trace overflow are not in it.
int ba_batch_spec_cells(BaBatch* b, uint64_t* cells) {
    if (!b || !cells) return fail("null argument");
    if (batch_results_refused(b, "speculative cells")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpy(cells, (const char*)b->prof.p + 60 * 8, 8, hipMemcpyDeviceToHost));
    return 0;
}
// Cells of the last run that were not computed: the padding columns of X-drop alignments' last blocks (ba_driver.hpp run(), the end clip).
// They are part of the pairs' `cells` -- the reference computes them --; the speculative cells of ba_batch_spec_cells keep counting full
// rectangles. 0 without X-drop, for byte-matrix and profile batches, in the special modes, and for a matrix that scores its padding byte at 0 or above.
int ba_batch_skipped_cells(BaBatch* b, uint64_t* cells) {
    if (!b || !cells) return fail("null argument");
    if (batch_results_refused(b, "skipped cells")) return 1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpy(cells, (const char*)b->prof.p + 61 * 8, 8, hipMemcpyDeviceToHost));
    return 0;
}
int ba_batch_kernel(BaBatch* b) {   // 0 the per-pair kernel (row-tiled class included), 1 k_multi, 2 k_quad beside it, 3 k_small
    if (!b) return -1;
    if (b->quad) return 2;
    const ba::KernelFamily f = family_of(b);
    return f == ba::FAM_SMALL ? 3 : ((f == ba::FAM_PAIR || f == ba::FAM_TILED) ? 0 : 1);
}
int ba_batch_geometry(BaBatch* b) { return !b ? -1 : (int)b->geom; }
int ba_batch_retried(BaBatch* b) { return b ? (int)b->retried : -1; }
int ba_batch_stats(BaBatch* b, BaAlignStats* out) {
    if (!b) return fail("null batch");
    if (!out) return fail("null argument");
    if (batch_stats_device(b, true)) return 1;
    HIP_TRY(hipMemcpy(out, b->stats.p, (size_t)b->n * sizeof(ba::AlignStats), hipMemcpyDeviceToHost));
    return 0;
}
int ba_batch_exact(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out) {
    return batch_exact(b, what, x_drop, which, n_which, out);
}
int ba_batch_exact_ms(BaBatch* b, float* ms, uint64_t* cells) {
    if (!b) return fail("null batch");
    if (ms) *ms = b->exact_ms;
    if (cells) *cells = b->exact_cells;
    return 0;
}
int ba_batch_exact_cigars(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out, uint64_t* run_off, uint32_t* runs,
                          uint64_t capacity) {
    return batch_exact_cigars(b, what, x_drop, which, n_which, out, run_off, runs, capacity);
}
int ba_batch_exact_cigars_ms(BaBatch* b, float* ms, uint64_t* cells) {
    if (!b) return fail("null batch");
    if (ms) *ms = b->xt_ms;
    if (cells) *cells = b->xt_cells;
    return 0;
}
// (the ba_*_exact_paths calls name a null out or run_off whatever the batch is)
static int exact_paths_args(const void* out, const void* run_off) {
    if (!out) return fail("null argument: out");
    if (!run_off) return fail("null argument: run_off");
    return 0;
}
int ba_batch_exact_paths(BaBatch* b, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExactPath* out, uint64_t* run_off, uint32_t* runs,
                         uintptr_t runs_cap) {
    if (exact_paths_args(out, run_off)) return 1;
    return batch_exact_cigars(b, what, x_drop, which, n_which, out, run_off, runs, runs_cap);
}
int ba_batch_exact_paths_ms(BaBatch* b, float* ms, uint64_t* cells) {
    if (!b) return fail("null batch");
    if (ms) *ms = b->xp_ms;
    if (cells) *cells = b->xp_cells;
    return 0;
}
int ba_exact_paths_check_lengths_profile(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n) {
    if (n && (!q_len || !r_len)) return fail("null argument");
    return exact_check_lengths(true, true, q_len, r_len, n, nullptr);
}
int ba_exact_trace_check_lengths(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n) {
    if (n && (!q_len || !r_len)) return fail("null argument");
    return exact_check_lengths(false, true, q_len, r_len, n, nullptr);
}
int ba_exact_check_lengths_profile(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n) {
    if (n && (!q_len || !r_len)) return fail("null argument");
    return exact_check_lengths(true, false, q_len, r_len, n, nullptr);
}
int ba_exact_check_lengths(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n) {
    if (n && (!q_len || !r_len)) return fail("null argument");
    return exact_check_lengths(false, false, q_len, r_len, n, nullptr);
}
int ba_accuracy_summary(const int32_t* score, const uint32_t* qidx, const uint32_t* ridx, const uint32_t* status, const BaExact* exact, uintptr_t n,
                        BaAccuracy* out) {
    if (!out) return fail("null argument: out");
    if (n && (!score || !exact)) return fail("null argument");
    BaAccuracy a{};
    a.n = n;
    double rel = 0; uint64_t rel_n = 0;
    for (size_t k = 0; k < n; k++) {
        if (status && (status[k] & ba::STATS_FAILED)) { a.skipped++; continue; }
        a.compared++;
        const int64_t diff = (int64_t)exact[k].score - score[k];
        if ((qidx && qidx[k] != exact[k].query_idx) || (ridx && ridx[k] != exact[k].reference_idx)) a.diff_end++;
        if (!diff) continue;
        const int32_t d32 = (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, diff));
        if (!a.wrong) a.min_diff = a.max_diff = d32;
        a.wrong++;
        if (diff > 0) a.below++; else a.above++;
        a.min_diff = std::min(a.min_diff, d32); a.max_diff = std::max(a.max_diff, d32);
        if (exact[k].score) { rel += (double)diff / std::fabs((double)exact[k].score); rel_n++; }
    }
    a.mean_rel_error = rel_n ? rel / (double)rel_n : 0.0;
    *out = a;
    return 0;
}
int ba_batch_text(BaBatch* b, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {
    if (!b) return fail("null batch");
    if (!offsets) return fail("null argument: offsets");
    return batch_text_device(b, what, offsets, text, capacity);
}
int ba_batch_text_ms(BaBatch* b, float* ms) {
    if (!b || !ms) return fail("null argument");
    *ms = b->text.ms;
    return 0;
}
int ba_batch_stats_ms(BaBatch* b, float* ms) {
    if (!b || !ms) return fail("null argument");
    *ms = b->stats_ms;
    return 0;
}
void ba_batch_destroy(BaBatch* b) { delete b; }

BaExtendBatch* ba_extend_batch_create(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                      const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                      const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, const uint8_t* strand, uintptr_t n_seeds) {
    ExtSet S;   // every argument is checked before the device is touched
    if (!matrix) { fail("null argument"); return nullptr; }
    if (spliced_check_params("extension", "extended", "a side ends where its score drops", kind, gaps, size, x_drop, mode) ||
        ext_plan(kind, pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand, n_seeds, S)) return nullptr;
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaExtendBatch> e(new BaExtendBatch);
    e->device = g_device; e->kind = kind; e->mode = mode;
    if (e->open(4) || ext_load(e.get(), S, n_seeds, matrix, gaps, size, x_drop, q_seed, r_seed, seed_len, true)) return nullptr;
    return e.release();
}
int ba_extend_batch_reload(BaExtendBatch* e, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                           const uint32_t* q_seed, const uint32_t* r_seed, const uint32_t* seed_len, const uint8_t* strand, uintptr_t n_seeds) {
    if (!e) return fail("null batch");
    ExtSet S;
    if (ext_plan(e->kind, pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand, n_seeds, S)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return ext_load(e, S, n_seeds, nullptr, Gaps{0, 0}, SizeRange{0, 0}, 0, q_seed, r_seed, seed_len, false);   // (matrix, gaps, range: the batch's own)
}
int ba_extend_batch_run(BaExtendBatch* e, float* kernel_ms) {
    if (!e) return fail("null batch");
    if (!e->n) return fail("no seeds loaded (the last reload failed)");
    HIP_TRY(hipSetDevice(e->device));
    e->ran = false; e->fill_ms = 0; e->splice_ms = 0; e->total_runs = 0;
    if (e->n_sides && batch_run(e->inner.get(), &e->fill_ms)) return 1;   // (re-runs included: the splice reads final results only)
    ba::ExtendParams ep = e->params();
    if (spliced_splice(e, [&] { return ba_launch_extend_results(e->stream, &ep); },   // (the launcher ends with its own offsets kernel)
                       [&] { ep.runs = e->runs.as<uint32_t>(); return ba_launch_extend_gather(e->stream, &ep); })) return 1;
    e->runs_done++;
    if (kernel_ms) *kernel_ms = e->fill_ms;
    return 0;
}
int ba_extend_batch_results(BaExtendBatch* e, int32_t* score, uint32_t* q_start, uint32_t* r_start, uint32_t* q_end, uint32_t* r_end,
                            int32_t* left_score, int32_t* right_score, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    return spliced_results(e, "extend_batch", score, q_start, r_start, q_end, r_end, left_score, right_score, cells, cigar_len, status);
}
int ba_extend_batch_cigars(BaExtendBatch* e, uint32_t* runs, uint64_t capacity) { return spliced_cigars(e, "extend_batch", runs, capacity); }
int ba_extend_batch_times(BaExtendBatch* e, float* fill_ms, float* pack_ms, float* splice_ms) {
    if (!e) return fail("null batch");
    if (fill_ms) *fill_ms = e->fill_ms;
    if (pack_ms) *pack_ms = e->pack_ms;
    if (splice_ms) *splice_ms = e->splice_ms;
    return 0;
}
int ba_extend_batch_stats(BaExtendBatch* e, BaAlignStats* out) {
    if (!e) return fail("null batch");
    if (!out) return fail("null argument");
    if (!(e->mode & BA_TRACE)) return fail("stats: the batch was created without BA_TRACE (the statistics are computed from the CIGAR runs)");
    if (!e->ran) return fail("stats: the batch has not finished a run (ba_extend_batch_run)");
    HIP_TRY(hipSetDevice(e->device));
    if (e->n_sides && batch_stats_device(e->inner.get(), false)) return 1;   // the sides' records, in the inner batch's device order
    if (!e->stats.p && e->stats.alloc((size_t)e->cap_n * sizeof(ba::AlignStats))) return 1;
    const ba::ExtendParams ep = e->params();
    HIP_TRY(ba_launch_stats_extend(e->stream, &ep, e->n_sides ? e->inner->stats.as<ba::AlignStats>() : nullptr, e->stats.as<ba::AlignStats>()));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, e->stats.p, (size_t)e->n * sizeof(ba::AlignStats), hipMemcpyDeviceToHost));
    return 0;
}
int ba_extend_batch_exact(BaExtendBatch* e, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* left, BaExact* right, int32_t* score) {
    return extend_exact(e, x_drop, which, n_which, left, right, score);
}
int ba_extend_batch_exact_paths(BaExtendBatch* e, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExactPath* out, BaExact* left, BaExact* right,
                                uint64_t* run_off, uint32_t* runs, uintptr_t runs_cap) {
    if (exact_paths_args(out, run_off)) return 1;
    return extend_exact_paths(e, x_drop, which, n_which, out, left, right, run_off, runs, runs_cap);
}
int ba_extend_batch_text(BaExtendBatch* e, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {
    return spliced_text(e, "ba_extend_batch_run", what, offsets, text, capacity);
}
void ba_extend_batch_destroy(BaExtendBatch* e) { delete e; }

BaChainBatch* ba_chain_batch_create(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                    const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, const uint64_t* anchor_first,
                                    const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len, const uint8_t* strand, uintptr_t n_chains) {
    ChainSet S;   // every argument is checked before the device is touched
    if (!matrix) { fail("null argument"); return nullptr; }
    if (spliced_check_params("chain", "chained", "the ends of a chain end where their score drops", kind, gaps, size, x_drop, mode) ||
        chain_plan(kind, pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand, n_chains, S)) return nullptr;
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaChainBatch> e(new BaChainBatch);
    e->device = g_device; e->kind = kind; e->mode = mode; e->gap_open = gaps.open; e->gap_extend = gaps.extend;
    if (e->open(4) || chain_load(e.get(), S, n_chains, matrix, gaps, size, x_drop, anchor_first, q_anchor, r_anchor, anchor_len, true)) return nullptr;
    return e.release();
}
int ba_chain_batch_reload(BaChainBatch* e, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                          const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len, const uint8_t* strand,
                          uintptr_t n_chains) {
    if (!e) return fail("null batch");
    ChainSet S;
    if (chain_plan(e->kind, pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand, n_chains, S)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return chain_load(e, S, n_chains, nullptr, Gaps{0, 0}, SizeRange{0, 0}, 0, anchor_first, q_anchor, r_anchor, anchor_len, false);   // (matrix, gaps, range: the batch's own)
}
int ba_chain_batch_run(BaChainBatch* e, float* kernel_ms) {
    if (!e) return fail("null batch");
    if (!e->n) return fail("no chains loaded (the last reload failed)");
    HIP_TRY(hipSetDevice(e->device));
    e->ran = false; e->ends_ms = 0; e->gaps_ms = 0; e->splice_ms = 0; e->total_runs = 0;
    // One fill after the other, each waited for: a traced launch holds waves that wait for one another and needs the device to itself to be
    // sure to end (ba_sized_batch_run). The splice reads final results only (re-runs included).
    if (e->n_ends && batch_run(e->ends.get(), &e->ends_ms)) return 1;
    if (e->n_gaps && batch_run(e->gaps.get(), &e->gaps_ms)) return 1;
    ba::ChainParams cp = e->params();
    auto results = [&]() -> hipError_t {   // ... and, for the gather, the offsets of the chains' runs
        const hipError_t r = ba_launch_chain_results(e->stream, &cp);
        return r != hipSuccess || !(e->mode & BA_TRACE) ? r : ba_launch_offsets(e->stream, cp.cigar_len, cp.out_off, cp.n);
    };
    if (spliced_splice(e, results, [&] { cp.runs = e->runs.as<uint32_t>(); return ba_launch_chain_gather(e->stream, &cp); })) return 1;
    e->runs_done++;
    if (kernel_ms) *kernel_ms = e->ends_ms + e->gaps_ms;
    return 0;
}
int ba_chain_batch_results(BaChainBatch* e, int32_t* score, uint32_t* q_start, uint32_t* r_start, uint32_t* q_end, uint32_t* r_end,
                           int32_t* left_score, int32_t* right_score, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    return spliced_results(e, "chain_batch", score, q_start, r_start, q_end, r_end, left_score, right_score, cells, cigar_len, status);
}
int ba_chain_batch_cigars(BaChainBatch* e, uint32_t* runs, uint64_t capacity) { return spliced_cigars(e, "chain_batch", runs, capacity); }
int ba_chain_batch_times(BaChainBatch* e, float* ends_ms, float* gaps_ms, float* pack_ms, float* splice_ms) {
    if (!e) return fail("null batch");
    if (ends_ms) *ends_ms = e->ends_ms;
    if (gaps_ms) *gaps_ms = e->gaps_ms;
    if (pack_ms) *pack_ms = e->pack_ms;
    if (splice_ms) *splice_ms = e->splice_ms;
    return 0;
}
int ba_chain_batch_stats(BaChainBatch* e, BaAlignStats* out) {
    if (!e) return fail("null batch");
    if (!out) return fail("null argument");
    if (!(e->mode & BA_TRACE)) return fail("stats: the batch was created without BA_TRACE (the statistics are computed from the CIGAR runs)");
    if (!e->ran) return fail("stats: the batch has not finished a run (ba_chain_batch_run)");
    HIP_TRY(hipSetDevice(e->device));
    e->stats_ms = 0;
    // the pieces' records, in the inner batches' device order
    if (e->n_ends && batch_stats_device(e->ends.get(), false)) return 1;
    if (e->n_gaps && batch_stats_device(e->gaps.get(), false)) return 1;
    if (!e->stats.p && e->stats.alloc((size_t)e->cap_n * sizeof(ba::AlignStats))) return 1;
    const ba::ChainParams cp = e->params();
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    HIP_TRY(ba_launch_stats_chain(e->stream, &cp, e->n_ends ? e->ends->stats.as<ba::AlignStats>() : nullptr,
                                  e->n_gaps ? e->gaps->stats.as<ba::AlignStats>() : nullptr, e->stats.as<ba::AlignStats>()));
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (e->elapsed(0, 1, &ms)) return 1;
    e->stats_ms = ms + (e->n_ends ? e->ends->stats_ms : 0) + (e->n_gaps ? e->gaps->stats_ms : 0);
    HIP_TRY(hipMemcpy(out, e->stats.p, (size_t)e->n * sizeof(ba::AlignStats), hipMemcpyDeviceToHost));
    return 0;
}
int ba_chain_batch_text(BaChainBatch* e, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {
    return spliced_text(e, "ba_chain_batch_run", what, offsets, text, capacity);
}
int ba_chain_batch_report_ms(BaChainBatch* e, float* stats_ms, float* text_ms) {
    if (!e) return fail("null batch");
    if (stats_ms) *stats_ms = e->stats_ms;
    if (text_ms) *text_ms = e->text.ms;
    return 0;
}
void ba_chain_batch_destroy(BaChainBatch* e) { delete e; }

// ------------------------------------------------------------------ colinear anchor chaining (ba_chaining_*)
// From a problem's raw hits to its best chains, in ba_chain_batch_create's layout (ba_chaining.hip; the rule: INTEGRATION.md, "Chaining
// anchors"). The host checks the arguments, orders the problems longest first and sizes the buffers; the recurrence, the picking and the
// gather are the device's.
// A sequence table ("Several sequences"): the sequence that holds position pos is the last non-empty one that starts at or before it.
struct SeqTable {
    const uint64_t* start; size_t n, last;   // n + 1 starts; the last non-empty sequence (0 when all are empty)
    SeqTable(const uint64_t* s, size_t n_seqs) : start(s), n(n_seqs), last(0) {
        for (size_t i = n; i-- > 0;) if (start[i + 1] > start[i]) { last = i; break; }
    }
    uint64_t total() const { return start[n]; }
    size_t of(uint64_t pos) const {   // (pos >= 0 = start[0]; an empty sequence starts where the next one does, so only trailing ones can come up)
        const size_t s = (size_t)(std::upper_bound(start, start + n, pos) - start) - 1;
        return s < last ? s : last;
    }
};
// the table of a call that gives lengths: between 1 and 2^20 sequences, less than 2^31 - 16 bytes in all
static int seq_table_from_len(const uint32_t* seq_len, size_t n_seqs, std::vector<uint64_t>& start) {
    if (n_seqs == 0 || n_seqs > (1u << 20)) return fail("an index must hold between 1 and 2^20 sequences (it has %llu)", (unsigned long long)n_seqs);
    start.assign(n_seqs + 1, 0);
    for (size_t s = 0; s < n_seqs; s++) start[s + 1] = start[s] + seq_len[s];
    if (start[n_seqs] >= ba::SEEDING_MAX_LEN) return fail("the sequences (%llu bytes in all) must be shorter than 2^31 - 16 bytes", (unsigned long long)start[n_seqs]);
    return 0;
}
struct BaChaining : StreamOwner {
    BaChainingParams P{};
    uint32_t n = 0, ring = 0;
    uint64_t n_anchors = 0, cap_n = 0, cap_anchors = 0, chains_cap = 0, total_chains = 0, total_kept = 0;
    DevBuf anchor_first, q_anchor, r_anchor, anchor_len, order, counter, f, pred, gain, mark, pos, cand_len, cand_score, n_chains, n_kept, chain_off, kept_off;
    DevBuf chain_problem, chain_rank, chain_score, out_first, out_q, out_r, out_len, out_src;
    float fill_ms = 0, pick_ms = 0, gather_ms = 0;
    bool ran = false;
    std::vector<uint64_t> seq_start;   // a bounded chainer's sequence table (ba_chaining_create_bounded, or a seeder's index's); empty otherwise
    DevBuf seq_start_dev;
    ba::ChainingParams params() const {
        ba::ChainingParams cp{};
        cp.n = n; cp.match_w = P.match_w; cp.drift_cost = P.drift_cost; cp.skip_cost = P.skip_cost; cp.lookback = P.lookback; cp.max_dist = P.max_dist;
        cp.bandwidth = P.bandwidth; cp.max_chains = P.max_chains; cp.min_score = P.min_score; cp.min_anchors = P.min_anchors; cp.ring = ring;
        cp.anchor_first = anchor_first.as<uint64_t>(); cp.q_anchor = q_anchor.as<uint32_t>(); cp.r_anchor = r_anchor.as<uint32_t>();
        cp.anchor_len = anchor_len.as<uint32_t>(); cp.order = order.as<uint32_t>(); cp.counter = counter.as<uint32_t>();
        cp.f = f.as<int32_t>(); cp.pred = pred.as<uint32_t>(); cp.gain = gain.as<uint32_t>(); cp.mark = mark.as<uint32_t>(); cp.pos = pos.as<uint32_t>();
        cp.cand_len = cand_len.as<uint32_t>(); cp.cand_score = cand_score.as<int32_t>(); cp.n_chains = n_chains.as<uint32_t>(); cp.n_kept = n_kept.as<uint32_t>();
        cp.chain_off = chain_off.as<uint64_t>(); cp.kept_off = kept_off.as<uint64_t>();
        cp.chain_problem = chain_problem.as<uint32_t>(); cp.chain_rank = chain_rank.as<uint32_t>(); cp.chain_score = chain_score.as<int32_t>();
        cp.out_first = out_first.as<uint64_t>(); cp.out_q = out_q.as<uint32_t>(); cp.out_r = out_r.as<uint32_t>(); cp.out_len = out_len.as<uint32_t>();
        cp.out_src = out_src.as<uint32_t>();
        if (!seq_start.empty()) { cp.n_seqs = (uint32_t)(seq_start.size() - 1); cp.seq_start = seq_start_dev.as<uint64_t>(); }
        return cp;
    }
};
static int chaining_check_params(const BaChainingParams& P) {
    if (P.match_w < 1) return fail("chaining: match_w must be at least 1 (it is %d)", P.match_w);
    if (P.drift_cost < 0 || P.skip_cost < 0) return fail("chaining: drift_cost and skip_cost must not be negative (they are %d and %d)", P.drift_cost, P.skip_cost);
    if (P.lookback < 1 || P.lookback > ba::CHAINING_MAX_LOOKBACK) return fail("chaining: lookback must be between 1 and %u (it is %u)", ba::CHAINING_MAX_LOOKBACK, P.lookback);
    if (P.max_dist < 1) return fail("chaining: max_dist must be at least 1");
    if (P.max_chains < 1 || P.max_chains > ba::CHAINING_MAX_CHAINS) return fail("chaining: max_chains must be between 1 and %u (it is %u)", ba::CHAINING_MAX_CHAINS, P.max_chains);
    if (P.min_anchors < 1) return fail("chaining: min_anchors must be at least 1");
    if ((uint64_t)P.drift_cost * P.bandwidth + (uint64_t)P.skip_cost * P.max_dist >= (1ull << 30))
        return fail("chaining: drift_cost * bandwidth + skip_cost * max_dist must stay below 2^30 (it is %llu)",
                    (unsigned long long)((uint64_t)P.drift_cost * P.bandwidth + (uint64_t)P.skip_cost * P.max_dist));
    return 0;
}
// Check a set of problems; -> the problems ordered by their number of anchors, the longest first.
// table: a bounded chainer's sequences -- every anchor ends at or before the end of the sequence that holds its start.
static int chaining_plan(const BaChainingParams& P, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len,
                         size_t n, std::vector<uint32_t>& order, const std::vector<uint64_t>* table = nullptr) {
    if (!anchor_first || !q_anchor || !r_anchor || !anchor_len) return fail("null argument");
    if (n == 0 || n > (1u << 28)) return fail("a chaining batch must hold between 1 and 2^28 problems");
    if (anchor_first[0] != 0) return fail("anchor_first must start at 0 (problem 0 starts at %llu)", (unsigned long long)anchor_first[0]);
    for (size_t p = 0; p < n; p++)
        if (anchor_first[p + 1] < anchor_first[p])
            return fail("problem %zu: anchor_first must not decrease (%llu after %llu)", p, (unsigned long long)anchor_first[p + 1], (unsigned long long)anchor_first[p]);
    if (anchor_first[n] > (1u << 28)) return fail("a chaining batch must hold at most 2^28 anchors");
    static const uint64_t none[2] = {0, 0};
    const SeqTable T(table ? table->data() : none, table ? table->size() - 1 : 1);
    for (size_t p = 0; p < n; p++) {
        uint64_t sum = 0, pq = 0, pr = 0;
        for (uint64_t a = anchor_first[p]; a < anchor_first[p + 1]; a++) {
            const uint64_t k = a - anchor_first[p], L = anchor_len[a], qe = (uint64_t)q_anchor[a] + L, re = (uint64_t)r_anchor[a] + L;
            if (L == 0) return fail("problem %zu, anchor %llu: anchor_len must be at least 1", p, (unsigned long long)k);
            if (qe >= (1ull << 31) || re >= (1ull << 31))
                return fail("problem %zu, anchor %llu: the anchor ends at query %llu, reference %llu: both must stay below 2^31", p, (unsigned long long)k,
                            (unsigned long long)qe, (unsigned long long)re);
            if (k && (re < pr || (re == pr && qe < pq)))
                return fail("problem %zu, anchor %llu: the anchors must be sorted by (reference end, query end): (%llu, %llu) comes after (%llu, %llu)", p,
                            (unsigned long long)k, (unsigned long long)re, (unsigned long long)qe, (unsigned long long)pr, (unsigned long long)pq);
            pq = qe; pr = re; sum += L;
            if (table) {
                const uint64_t end = r_anchor[a] < T.total() ? T.start[T.of(r_anchor[a]) + 1] : T.total();
                if (re > end)
                    return fail("problem %zu, anchor %llu: the anchor covers reference %llu to %llu and leaves its sequence, which ends at %llu", p,
                                (unsigned long long)k, (unsigned long long)r_anchor[a], (unsigned long long)re, (unsigned long long)end);
            }
        }
        if (sum * (uint64_t)P.match_w >= (1ull << 31))
            return fail("problem %zu: match_w * the sum of anchor_len must stay below 2^31 (it is %llu)", p, (unsigned long long)(sum * (uint64_t)P.match_w));
    }
    order.resize(n);
    for (size_t p = 0; p < n; p++) order[p] = (uint32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return anchor_first[a + 1] - anchor_first[a] > anchor_first[b + 1] - anchor_first[b]; });
    return 0;
}
// (the three anchor arrays are host arrays, or with from = hipMemcpyDeviceToDevice arrays on the batch's device: ba_chaining_create_seeded)
static int chaining_load(BaChaining* e, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len, size_t n,
                         const std::vector<uint32_t>& order, bool create, hipMemcpyKind from = hipMemcpyHostToDevice) {
    const uint64_t na = anchor_first[n];
    if (create) {
        e->cap_n = n; e->cap_anchors = na;
        DevBuf* per_anchor4[] = {&e->q_anchor, &e->r_anchor, &e->anchor_len, &e->f, &e->pred, &e->gain, &e->mark, &e->pos, &e->out_q, &e->out_r, &e->out_len, &e->out_src};
        for (DevBuf* d : per_anchor4) if (d->alloc(na * 4)) return 1;
        if (e->anchor_first.alloc((n + 1) * 8) || e->order.alloc(n * 4) || e->counter.alloc(4) || e->cand_len.alloc(n * e->P.max_chains * 4) ||
            e->cand_score.alloc(n * e->P.max_chains * 4) || e->n_chains.alloc(n * 4) || e->n_kept.alloc(n * 4) || e->chain_off.alloc((n + 1) * 8) ||
            e->kept_off.alloc((n + 1) * 8)) return 1;
    } else {
        if (n > e->cap_n) return fail("reload: %zu problems exceed the batch's capacity of %llu", n, (unsigned long long)e->cap_n);
        if (na > e->cap_anchors) return fail("reload: %llu anchors exceed the batch's capacity of %llu", (unsigned long long)na, (unsigned long long)e->cap_anchors);
    }
    e->n = 0; e->ran = false;   // (a failure from here on leaves no problems loaded)
    if (h2d(e->anchor_first, anchor_first, n + 1) || h2d(e->order, order.data(), n)) return 1;
    if (na) {
        if (from == hipMemcpyDeviceToDevice) {
            // on the batch's own stream, which its kernels follow, and waited for: a device-to-device hipMemcpy need not have finished when it
            // returns, and the source may be reloaded or freed as soon as this call is over
            HIP_TRY(hipMemcpyAsync(e->q_anchor.p, q_anchor, na * 4, from, e->stream));
            HIP_TRY(hipMemcpyAsync(e->r_anchor.p, r_anchor, na * 4, from, e->stream));
            HIP_TRY(hipMemcpyAsync(e->anchor_len.p, anchor_len, na * 4, from, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else if (h2d(e->q_anchor, q_anchor, na) || h2d(e->r_anchor, r_anchor, na) || h2d(e->anchor_len, anchor_len, na)) return 1;
    }
    e->n = (uint32_t)n; e->n_anchors = na;
    return 0;
}
// the sequence table of a bounded chainer goes to the device once, at its creation
static int chaining_bound(BaChaining* e, const std::vector<uint64_t>& table) {
    e->seq_start = table;
    return e->seq_start_dev.alloc(table.size() * 8) || h2d(e->seq_start_dev, table.data(), table.size());
}
static BaChaining* chaining_create(const BaChainingParams* params, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                                   const uint32_t* anchor_len, size_t n_problems, const std::vector<uint64_t>* table) {
    std::vector<uint32_t> order;   // every argument is checked before the device is touched
    if (chaining_check_params(*params) || chaining_plan(*params, anchor_first, q_anchor, r_anchor, anchor_len, n_problems, order, table)) return nullptr;
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaChaining> e(new BaChaining);
    e->device = g_device; e->P = *params;
    e->ring = 128;
    while (e->ring < params->lookback + 64u) e->ring <<= 1;
    if (e->open(4) || (table && chaining_bound(e.get(), *table)) ||
        chaining_load(e.get(), anchor_first, q_anchor, r_anchor, anchor_len, n_problems, order, true)) return nullptr;
    return e.release();
}
BaChaining* ba_chaining_create(const BaChainingParams* params, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                               const uint32_t* anchor_len, uintptr_t n_problems) {
    if (!params) { fail("null argument"); return nullptr; }
    return chaining_create(params, anchor_first, q_anchor, r_anchor, anchor_len, n_problems, nullptr);
}
BaChaining* ba_chaining_create_bounded(const BaChainingParams* params, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor,
                                       const uint32_t* anchor_len, uintptr_t n_problems, const uint64_t* seq_start, uintptr_t n_seqs) {
    if (!params || !seq_start) { fail("null argument"); return nullptr; }
    if (n_seqs == 0 || n_seqs > (1u << 20)) { fail("a sequence table must hold between 1 and 2^20 sequences (it has %llu)", (unsigned long long)n_seqs); return nullptr; }
    if (seq_start[0] != 0) { fail("seq_start must start at 0 (sequence 0 starts at %llu)", (unsigned long long)seq_start[0]); return nullptr; }
    for (size_t s = 0; s < n_seqs; s++)
        if (seq_start[s + 1] < seq_start[s]) {
            fail("sequence %zu: seq_start must not decrease (%llu after %llu)", s, (unsigned long long)seq_start[s + 1], (unsigned long long)seq_start[s]);
            return nullptr;
        }
    if (seq_start[n_seqs] >= ba::SEEDING_MAX_LEN) {
        fail("the sequences (%llu bytes in all) must be shorter than 2^31 - 16 bytes", (unsigned long long)seq_start[n_seqs]);
        return nullptr;
    }
    const std::vector<uint64_t> table(seq_start, seq_start + n_seqs + 1);
    return chaining_create(params, anchor_first, q_anchor, r_anchor, anchor_len, n_problems, &table);
}
int ba_chaining_reload(BaChaining* e, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len,
                       uintptr_t n_problems) {
    if (!e) return fail("null batch");
    std::vector<uint32_t> order;
    if (chaining_plan(e->P, anchor_first, q_anchor, r_anchor, anchor_len, n_problems, order, e->seq_start.empty() ? nullptr : &e->seq_start)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return chaining_load(e, anchor_first, q_anchor, r_anchor, anchor_len, n_problems, order, false);
}
int ba_chaining_run(BaChaining* e, float* kernel_ms) {
    if (!e) return fail("null batch");
    if (!e->n) return fail("no problems loaded (the last reload failed)");
    HIP_TRY(hipSetDevice(e->device));
    e->ran = false; e->fill_ms = e->pick_ms = e->gather_ms = 0; e->total_chains = e->total_kept = 0;
    ba::ChainingParams cp = e->params();
    HIP_TRY(hipMemsetAsync(e->counter.p, 0, 4, e->stream));
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    if (cp.n_seqs) HIP_TRY(ba_launch_chaining_fill_bounded(e->stream, &cp));   // (a chainer with a sequence table)
    else HIP_TRY(ba_launch_chaining_fill(e->stream, &cp));
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(ba_launch_chaining_pick(e->stream, &cp));
    HIP_TRY(ba_launch_offsets(e->stream, cp.n_chains, e->chain_off.as<uint64_t>(), cp.n));
    HIP_TRY(ba_launch_offsets(e->stream, cp.n_kept, e->kept_off.as<uint64_t>(), cp.n));
    HIP_TRY(hipEventRecord(e->ev[2], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->elapsed(0, 1, &e->fill_ms) || e->elapsed(1, 2, &e->pick_ms)) return 1;
    uint64_t chains = 0, kept = 0;
    HIP_TRY(hipMemcpy(&chains, e->chain_off.as<uint64_t>() + e->n, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&kept, e->kept_off.as<uint64_t>() + e->n, 8, hipMemcpyDeviceToHost));
    if (chains > (uint64_t)e->n * e->P.max_chains || kept > e->n_anchors)
        return fail("chaining: the device counted %llu chains and %llu anchors, more than the set can hold", (unsigned long long)chains, (unsigned long long)kept);
    if (chains > e->chains_cap || !e->out_first.p) {   // (grows, never shrinks)
        if (e->chain_problem.alloc(chains * 4) || e->chain_rank.alloc(chains * 4) || e->chain_score.alloc(chains * 4) || e->out_first.alloc((chains + 1) * 8)) return 1;
        e->chains_cap = chains;
        cp = e->params();
    }
    HIP_TRY(hipEventRecord(e->ev[2], e->stream));
    HIP_TRY(ba_launch_chaining_gather(e->stream, &cp));
    HIP_TRY(hipEventRecord(e->ev[3], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->elapsed(2, 3, &e->gather_ms)) return 1;
    e->total_chains = chains; e->total_kept = kept;
    e->ran = true;
    if (kernel_ms) *kernel_ms = e->fill_ms + e->pick_ms + e->gather_ms;
    return 0;
}
int ba_chaining_counts(BaChaining* e, uint64_t* n_chains, uint64_t* n_anchors, uint32_t* chains_per_problem) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_chaining_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    if (n_chains) *n_chains = e->total_chains;
    if (n_anchors) *n_anchors = e->total_kept;
    return d2h(e->n_chains, chains_per_problem, e->n);
}
int ba_chaining_results(BaChaining* e, uint32_t* chain_problem, uint32_t* chain_rank, int32_t* chain_score, uint64_t* out_anchor_first, uint32_t* out_q_anchor,
                        uint32_t* out_r_anchor, uint32_t* out_anchor_len, uint32_t* out_anchor_src) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_chaining_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    const size_t nc = e->total_chains, nk = e->total_kept;
    if (d2h(e->chain_problem, chain_problem, nc) || d2h(e->chain_rank, chain_rank, nc) || d2h(e->chain_score, chain_score, nc) ||
        d2h(e->out_first, out_anchor_first, nc + 1) || d2h(e->out_q, out_q_anchor, nk) || d2h(e->out_r, out_r_anchor, nk) ||
        d2h(e->out_len, out_anchor_len, nk) || d2h(e->out_src, out_anchor_src, nk)) return 1;
    return 0;
}
int ba_chaining_dp(BaChaining* e, int32_t* f, int32_t* pred) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_chaining_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    if (d2h(e->f, f, e->n_anchors)) return 1;
    if (pred) HIP_TRY(hipMemcpy(pred, e->pred.p, e->n_anchors * 4, hipMemcpyDeviceToHost));   // (CHAINING_NONE is -1)
    return 0;
}
int ba_chaining_times(BaChaining* e, float* fill_ms, float* pick_ms, float* gather_ms) {
    if (!e) return fail("null batch");
    if (fill_ms) *fill_ms = e->fill_ms;
    if (pick_ms) *pick_ms = e->pick_ms;
    if (gather_ms) *gather_ms = e->gather_ms;
    return 0;
}
void ba_chaining_destroy(BaChaining* e) { delete e; }

// ------------------------------------------------------------------ minimizer seeding (ba_seeding_*)
// From the bytes of a problem to its raw hits, in the order ba_chaining_create demands (ba_seeding.hip; the rule: INTEGRATION.md,
// "Seeding"). The host checks the arguments, orders sequences and problems longest first and sizes the buffers between the passes; the
// sketch, the sort and the match are the device's. The three kinds of seeder -- problems with a reference each, problems against a
// reference index, reads against a canonical index on both strands at once (the two sections on the index, below) -- are one BaSeeding,
// loaded by seeding_load and run by ba_seeding_run: a kind is a set's counts, its kernels and the wording of two messages.
struct SeedingSet {   // a checked set of problems: the extent of its sequences in the caller's pool, the per-sequence arrays, the orders
    const uint8_t* lo = nullptr; uint64_t bytes = 0;
    // the sequences that are sketched (the queries, then the references; a both-strand set: the reads), the queries whose keys are sorted,
    // the entries of match_order, the problems; what a reload that holds too many of them calls them
    size_t n_seqs = 0, n_sort = 0, n_match = 0, n_problems = 0;
    const char* nouns = "problems";
    std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<uint8_t> rc;   // n_seqs each; rc: empty when no sequence has a strand
    // seq_order: n_seqs, and empty when the sequences are the queries, which sort_order lists. match_order: the problems for the match, or
    // against an index for the sort of the hits
    std::vector<uint32_t> seq_order, sort_order, match_order;
};
struct IndexData {   // a reference index on the device (ba_ref_index_*): shared by the index and the seeders made from it, freed with the last
    int device = 0;
    uint32_t k = 0, w = 0, prefix_bits = 0, longest_run = 0;
    uint64_t ref_len = 0, n_entries = 0;
    DevBuf key, table;   // n_entries keys code << 32 | pos, ascending; (1 << prefix_bits) + 1 bounds
    // the sequences, laid end to end in the frame of the positions: where each starts, and where the last one ends (one entry more than
    // sequences). multi: made by ba_ref_index_create_multi, so chainers over its seeders' hits are bounded by this table.
    std::vector<uint64_t> seq_start;
    bool multi = false;
    bool canonical = false;   // made by ba_ref_index_create_canonical ("Both strands at once"): the keys are code << 32 | strand << 31 | pos
};
struct BaSeeding : StreamOwner {
    BaSeedingParams P{};
    uint32_t n = 0, n_seqs = 0, n_reads = 0;   // the problems, the sequences that are sketched, the queries (the counts of the loaded SeedingSet)
    uint64_t cap_n = 0, cap_raw = 0, seeds_cap = 0, q_seeds_cap = 0, hits_cap = 0, n_q_seeds = 0, n_seeds = 0, n_hits = 0;
    DevBuf raw, seq_off, seq_len, seq_rc, seq_order, sort_order, match_order, counter, seed_cnt, seed_first, seed_pos, seed_code, q_key, hit_cnt, hit_first,
           q_hit, r_hit, hit_len;
    std::shared_ptr<const IndexData> index;   // an indexed seeder (ba_seeding_create_indexed): every problem's reference is the index's
    uint32_t max_ref_occ = 0;
    DevBuf hit_key;                           // ... its hits as sort keys, as large as the hit arrays
    // a both-strand seeder (ba_seeding_create_indexed_both): n_reads reads, each sketched once, and n = 2 n_reads problems. The per-sequence
    // arrays, seed_cnt and seed_first are the reads' (n_reads), hit_cnt and hit_first the problems'; seq_order is a view of sort_order,
    // match_order lists both problems of a read together, and cap_n counts reads.
    bool both = false;
    float sketch_ms = 0, sort_ms = 0, match_ms = 0;
    bool ran = false;
    ba::IndexBothParams both_params() const {
        ba::IndexBothParams bp{};
        bp.lp = lookup_params();
        bp.lp.n = n_reads; bp.lp.order = sort_order.as<uint32_t>();   // (the lookup goes read by read, the sort of the hits problem by problem)
        bp.q_len = seq_len.as<uint32_t>();
        return bp;
    }
    ba::IndexLookupParams lookup_params() const {
        ba::IndexLookupParams lp{};
        lp.n = n; lp.k = P.k; lp.max_occ = P.max_occ; lp.max_ref_occ = max_ref_occ;
        lp.prefix_bits = index->prefix_bits; lp.n_entries = (uint32_t)index->n_entries;
        lp.order = match_order.as<uint32_t>(); lp.seed_first = seed_first.as<uint64_t>(); lp.q_key = q_key.as<uint64_t>();
        lp.key = index->key.as<uint64_t>(); lp.table = index->table.as<uint32_t>();
        lp.hit_cnt = hit_cnt.as<uint32_t>(); lp.hit_first = hit_first.as<uint64_t>(); lp.hit_key = hit_key.as<uint64_t>();
        lp.q_hit = q_hit.as<uint32_t>(); lp.r_hit = r_hit.as<uint32_t>(); lp.hit_len = hit_len.as<uint32_t>();
        return lp;
    }
    ba::SeedingParams params() const {
        ba::SeedingParams sp{};
        sp.n = n_reads; sp.k = P.k; sp.w = P.w; sp.max_occ = P.max_occ;
        sp.pool = raw.as<uint8_t>(); sp.seq_off = seq_off.as<uint64_t>(); sp.seq_len = seq_len.as<uint32_t>(); sp.seq_rc = seq_rc.as<uint8_t>();
        sp.seq_order = seq_order.as<uint32_t>(); sp.sort_order = sort_order.as<uint32_t>(); sp.match_order = match_order.as<uint32_t>();
        sp.counter = counter.as<uint32_t>(); sp.seed_cnt = seed_cnt.as<uint32_t>(); sp.seed_first = seed_first.as<uint64_t>();
        sp.seed_pos = seed_pos.as<uint32_t>(); sp.seed_code = seed_code.as<uint32_t>(); sp.q_key = q_key.as<uint64_t>();
        sp.hit_cnt = hit_cnt.as<uint32_t>(); sp.hit_first = hit_first.as<uint64_t>();
        sp.q_hit = q_hit.as<uint32_t>(); sp.r_hit = r_hit.as<uint32_t>(); sp.hit_len = hit_len.as<uint32_t>();
        return sp;
    }
};
static int seeding_check_params(const BaSeedingParams& P) {
    if (P.k < ba::SEEDING_MIN_K || P.k > ba::SEEDING_MAX_K) return fail("seeding: k must be between %u and %u (it is %u)", ba::SEEDING_MIN_K, ba::SEEDING_MAX_K, P.k);
    if (P.w < 1 || P.w > ba::SEEDING_MAX_W) return fail("seeding: w must be between 1 and %u (it is %u)", ba::SEEDING_MAX_W, P.w);
    if (P.max_occ < 1) return fail("seeding: max_occ must be at least 1");
    return 0;
}
// Check a set of problems; -> the per-sequence arrays (offsets relative to the lowest byte any sequence has) and the three orders.
// indexed: the problems of an indexed seeder, reads against a reference index: r_off and r_len are not read, every reference is empty.
static int seeding_plan(const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, const uint8_t* strand,
                        size_t n, SeedingSet& S, bool indexed = false) {
    if (!pool || !q_off || !q_len || (!indexed && (!r_off || !r_len))) return fail("null argument");
    if (n == 0 || n > (1u << 28)) return fail("a seeding batch must hold between 1 and 2^28 problems");
    S = SeedingSet();
    S.n_seqs = 2 * n; S.n_sort = S.n_match = S.n_problems = n;
    S.off.resize(2 * n); S.len.resize(2 * n); S.rc.assign(2 * n, 0);
    const uint8_t* hi = nullptr;
    for (size_t p = 0; p < n; p++) {
        const uint8_t st = strand ? strand[p] : 0;
        if (st > 1) return fail("problem %zu: strand must be 0 or 1", p);
        const uint32_t rl = indexed ? 0u : r_len[p];
        if (q_len[p] >= ba::SEEDING_MAX_LEN || rl >= ba::SEEDING_MAX_LEN)
            return fail("problem %zu: the sequences (query %u, reference %u bytes) must be shorter than 2^31 - 16 bytes", p, q_len[p], rl);
        // (an empty sequence names no byte: whatever its offset, it does not widen what is uploaded)
        if (q_len[p]) { const uint8_t* q = pool + q_off[p]; if (!S.lo || q < S.lo) S.lo = q; if (!hi || q + q_len[p] > hi) hi = q + q_len[p]; }
        if (rl) { const uint8_t* r = pool + r_off[p]; if (!S.lo || r < S.lo) S.lo = r; if (!hi || r + rl > hi) hi = r + rl; }
        S.off[p] = q_off[p]; S.off[n + p] = rl ? r_off[p] : 0;
        S.len[p] = q_len[p]; S.len[n + p] = rl;
        S.rc[p] = st;
    }
    const uint64_t base = S.lo ? (uint64_t)(S.lo - pool) : 0;
    for (size_t s = 0; s < 2 * n; s++) S.off[s] = S.len[s] ? S.off[s] - base : 0;
    S.bytes = S.lo ? (uint64_t)(hi - S.lo) : 0;
    auto by = [](const uint32_t* len, std::vector<uint32_t>& order, size_t m) {
        order.resize(m);
        for (size_t i = 0; i < m; i++) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
    };
    by(S.len.data(), S.seq_order, 2 * n);
    by(q_len, S.sort_order, n);
    if (indexed) S.match_order = S.sort_order;   // (the lookup and the sort of the hits: longest query first)
    else by(S.len.data() + n, S.match_order, n);
    return 0;
}
// Size the per-sequence and per-problem arrays for the set (create) or admit it to them (a reload), and upload it.
static int seeding_load(BaSeeding* e, const SeedingSet& S, bool create) {
    const size_t ns = S.n_seqs, nq = S.n_sort, nm = S.n_match, np = S.n_problems;
    if (create) {
        e->cap_n = nq; e->cap_raw = S.bytes;
        if (e->raw.alloc(S.bytes) || e->seq_off.alloc(ns * 8) || e->seq_len.alloc(ns * 4) || (!S.rc.empty() && e->seq_rc.alloc(ns)) ||
            e->sort_order.alloc(nq * 4) || e->match_order.alloc(nm * 4) || e->counter.alloc(4) || e->seed_cnt.alloc(ns * 4) ||
            e->seed_first.alloc((ns + 1) * 8) || e->hit_cnt.alloc(np * 4) || e->hit_first.alloc((np + 1) * 8)) return 1;
        if (S.seq_order.empty()) e->seq_order.view(e->sort_order.p, nq * 4);
        else if (e->seq_order.alloc(ns * 4)) return 1;
    } else {
        if (nq > e->cap_n) return fail("reload: %zu %s exceed the batch's capacity of %llu", nq, S.nouns, (unsigned long long)e->cap_n);
        if (S.bytes > e->cap_raw) return fail("reload: %llu sequence bytes exceed the batch's capacity of %llu", (unsigned long long)S.bytes, (unsigned long long)e->cap_raw);
    }
    e->n = e->n_seqs = e->n_reads = 0; e->ran = false;   // (a failure from here on leaves no problems loaded)
    if ((S.bytes && h2d(e->raw, S.lo, S.bytes)) || h2d(e->seq_off, S.off.data(), ns) || h2d(e->seq_len, S.len.data(), ns) ||
        (!S.rc.empty() && h2d(e->seq_rc, S.rc.data(), ns)) || (!S.seq_order.empty() && h2d(e->seq_order, S.seq_order.data(), ns)) ||
        h2d(e->sort_order, S.sort_order.data(), nq) || h2d(e->match_order, S.match_order.data(), nm)) return 1;
    e->n = (uint32_t)np; e->n_seqs = (uint32_t)ns; e->n_reads = (uint32_t)nq;
    return 0;
}
BaSeeding* ba_seeding_create(const BaSeedingParams* params, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off,
                             const uint32_t* r_len, const uint8_t* strand, uintptr_t n_problems) {
    SeedingSet S;   // every argument is checked before the device is touched
    if (!params) { fail("null argument"); return nullptr; }
    if (seeding_check_params(*params) || seeding_plan(pool, q_off, q_len, r_off, r_len, strand, n_problems, S)) return nullptr;
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaSeeding> e(new BaSeeding);
    e->device = g_device; e->P = *params;
    if (e->open(9) || seeding_load(e.get(), S, true)) return nullptr;
    return e.release();
}
int ba_seeding_reload(BaSeeding* e, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                      const uint8_t* strand, uintptr_t n_problems) {
    if (!e) return fail("null batch");
    if (e->both) return fail("ba_seeding_reload: the seeder takes its reads on both strands at once; call ba_seeding_reload_indexed_both");
    if (e->index) return fail("ba_seeding_reload: the seeder was created over a reference index; call ba_seeding_reload_indexed");
    SeedingSet S;
    if (seeding_plan(pool, q_off, q_len, r_off, r_len, strand, n_problems, S)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return seeding_load(e, S, false);
}
// More than 2^28 hits after the count pass, so no emit: name the first problem that does not fit what the ones before it left.
static int seeding_over_limit(const BaSeeding* e) {
    const size_t n = e->n;
    std::vector<uint32_t> per(n);
    HIP_TRY(hipMemcpy(per.data(), e->hit_cnt.p, n * 4, hipMemcpyDeviceToHost));
    uint64_t left = ba::SEEDING_MAX_HITS;
    size_t p = 0;
    while (p + 1 < n && per[p] <= left) left -= per[p++];
    const char* at_least = per[p] == 0xffffffffu ? "at least " : "";
    if (e->both)
        return fail("seeding: the set has more than 2^28 hits: read %zu on strand %zu alone has %s%u, with %llu left after the problems before it; lower "
                    "max_occ (it is %u) or max_ref_occ (it is %u), or seed fewer reads at once", p / 2, p % 2, at_least, per[p], (unsigned long long)left,
                    e->P.max_occ, e->max_ref_occ);
    return fail("seeding: the set has more than 2^28 hits: problem %zu alone has %s%u, with %llu left after the problems before it; lower max_occ "
                "(it is %u) or seed fewer problems at once", p, at_least, per[p], (unsigned long long)left, e->P.max_occ);
}
// Every kind of seeder: the sketch (count, scan, emit), the sort of every query's keys, the match (count, scan over the problems, emit)
// and, against an index, the sort of every problem's hits. What a kind chooses is taken from the seeder here at the top; the events, the
// two sizings between the passes, the refusal and the times are written once.
int ba_seeding_run(BaSeeding* e, float* kernel_ms) {
    if (!e) return fail("null batch");
    if (!e->n) return fail("no problems loaded (the last reload failed)");
    HIP_TRY(hipSetDevice(e->device));
    e->ran = false; e->sketch_ms = e->sort_ms = e->match_ms = 0; e->n_q_seeds = e->n_seeds = e->n_hits = 0;
    const uint32_t n = e->n, n_seqs = e->n_seqs, n_reads = e->n_reads;
    const bool indexed = (bool)e->index;   // the lookup in the index in place of the match; its emit pass writes sort keys
    const auto sketch = e->both ? ba_launch_both_read_sketch : ba_launch_seeding_sketch;
    ba::SeedingParams sp = e->params();
    const auto match = [&](int emit) {   // (the parameters are read at the call: the buffers they name grow between the passes)
        if (!indexed) return ba_launch_seeding_match(e->stream, &sp, emit);
        if (e->both) { const ba::IndexBothParams bp = e->both_params(); return ba_launch_both_lookup(e->stream, &bp, emit); }
        const ba::IndexLookupParams lp = e->lookup_params();
        return ba_launch_index_lookup(e->stream, &lp, emit);
    };
    // the sketch: count, scan, emit
    HIP_TRY(hipMemsetAsync(e->counter.p, 0, 4, e->stream));
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    HIP_TRY(sketch(e->stream, &sp, 0));
    HIP_TRY(ba_launch_offsets(e->stream, sp.seed_cnt, e->seed_first.as<uint64_t>(), n_seqs));
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    uint64_t q_seeds = 0, seeds = 0;
    HIP_TRY(hipMemcpy(&seeds, e->seed_first.as<uint64_t>() + n_seqs, 8, hipMemcpyDeviceToHost));
    if (n_seqs == n_reads) q_seeds = seeds;   // (no sequence but the queries)
    else HIP_TRY(hipMemcpy(&q_seeds, e->seed_first.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost));
    if (seeds > e->seeds_cap || !e->seed_pos.p) {   // (grow, never shrink)
        if (e->seed_pos.alloc(seeds * 4) || e->seed_code.alloc(seeds * 4)) return 1;
        e->seeds_cap = seeds;
    }
    if (q_seeds > e->q_seeds_cap || !e->q_key.p) {
        if (e->q_key.alloc(q_seeds * 8)) return 1;
        e->q_seeds_cap = q_seeds;
    }
    sp = e->params();
    HIP_TRY(hipMemsetAsync(e->counter.p, 0, 4, e->stream));
    HIP_TRY(hipEventRecord(e->ev[2], e->stream));
    HIP_TRY(sketch(e->stream, &sp, 1));
    HIP_TRY(hipEventRecord(e->ev[3], e->stream));
    // the sort of the queries' keys (a both-strand read's: the order of the keys puts a code's strand-0 entries first); the match: count, scan
    HIP_TRY(ba_launch_seeding_sort(e->stream, &sp));
    HIP_TRY(hipEventRecord(e->ev[4], e->stream));
    HIP_TRY(match(0));
    HIP_TRY(ba_launch_offsets(e->stream, sp.hit_cnt, e->hit_first.as<uint64_t>(), n));
    HIP_TRY(hipEventRecord(e->ev[5], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    uint64_t hits = 0;
    HIP_TRY(hipMemcpy(&hits, e->hit_first.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
    if (hits > ba::SEEDING_MAX_HITS) return seeding_over_limit(e);
    if (hits > e->hits_cap || !e->q_hit.p) {
        if (e->q_hit.alloc(hits * 4) || e->r_hit.alloc(hits * 4) || e->hit_len.alloc(hits * 4) || (indexed && e->hit_key.alloc(hits * 8))) return 1;
        e->hits_cap = hits;
    }
    sp = e->params();
    // the match: emit; the sort of every problem's keys unpacks them
    HIP_TRY(hipEventRecord(e->ev[6], e->stream));
    HIP_TRY(match(1));
    HIP_TRY(hipEventRecord(e->ev[7], e->stream));
    if (indexed) { const ba::IndexLookupParams lp = e->lookup_params(); HIP_TRY(ba_launch_index_hit_sort(e->stream, &lp)); }
    HIP_TRY(hipEventRecord(e->ev[8], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float a = 0, b = 0;
    if (e->elapsed(0, 1, &a) || e->elapsed(2, 3, &b)) return 1;
    e->sketch_ms = a + b;
    if (e->elapsed(3, 4, &a) || e->elapsed(7, 8, &b)) return 1;
    e->sort_ms = indexed ? a + b : a;   // ... and the sort of the hits
    if (e->elapsed(4, 5, &a) || e->elapsed(6, 7, &b)) return 1;
    e->match_ms = a + b;
    e->n_q_seeds = q_seeds; e->n_seeds = seeds; e->n_hits = hits;
    e->ran = true;
    if (kernel_ms) *kernel_ms = e->sketch_ms + e->sort_ms + e->match_ms;
    return 0;
}
int ba_seeding_counts(BaSeeding* e, uint64_t* n_hits, uint64_t* n_q_seeds, uint64_t* n_r_seeds, uint32_t* hits_per_problem) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_seeding_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    if (n_hits) *n_hits = e->n_hits;
    if (n_q_seeds) *n_q_seeds = e->n_q_seeds;
    if (n_r_seeds) *n_r_seeds = e->n_seeds - e->n_q_seeds;
    return d2h(e->hit_cnt, hits_per_problem, e->n);
}
int ba_seeding_results(BaSeeding* e, uint64_t* hit_first, uint32_t* q_hit, uint32_t* r_hit, uint32_t* hit_len) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_seeding_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    if (d2h(e->hit_first, hit_first, (size_t)e->n + 1) || d2h(e->q_hit, q_hit, e->n_hits) || d2h(e->r_hit, r_hit, e->n_hits) ||
        d2h(e->hit_len, hit_len, e->n_hits)) return 1;
    return 0;
}
int ba_seeding_sketch(BaSeeding* e, uint64_t* q_seed_first, uint32_t* q_seed_pos, uint32_t* q_seed_code, uint64_t* r_seed_first, uint32_t* r_seed_pos,
                      uint32_t* r_seed_code) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_seeding_run has not been called");
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = e->n_reads, nq = e->n_q_seeds, nr = e->n_seeds - e->n_q_seeds;
    if (d2h(e->seed_first, q_seed_first, n + 1) || d2h(e->seed_pos, q_seed_pos, nq) || d2h(e->seed_code, q_seed_code, nq)) return 1;
    if (e->both) {   // per read, and no reference entries: seed_first holds the reads' offsets only
        if (r_seed_first) std::fill(r_seed_first, r_seed_first + n + 1, 0ull);
        return 0;
    }
    if (r_seed_first) {   // (the references' entries lie behind the queries')
        HIP_TRY(hipMemcpy(r_seed_first, e->seed_first.as<uint64_t>() + n, (n + 1) * 8, hipMemcpyDeviceToHost));
        for (size_t p = 0; p <= n; p++) r_seed_first[p] -= nq;
    }
    if (r_seed_pos) HIP_TRY(hipMemcpy(r_seed_pos, e->seed_pos.as<uint32_t>() + nq, nr * 4, hipMemcpyDeviceToHost));
    if (r_seed_code) HIP_TRY(hipMemcpy(r_seed_code, e->seed_code.as<uint32_t>() + nq, nr * 4, hipMemcpyDeviceToHost));
    return 0;
}
int ba_seeding_times(BaSeeding* e, float* sketch_ms, float* sort_ms, float* match_ms) {
    if (!e) return fail("null batch");
    if (sketch_ms) *sketch_ms = e->sketch_ms;
    if (sort_ms) *sort_ms = e->sort_ms;
    if (match_ms) *match_ms = e->match_ms;
    return 0;
}
int ba_seeding_problems(BaSeeding* e, uint64_t* n_problems, uint64_t* n_reads) {
    if (!e) return fail("null batch");
    if (n_problems) *n_problems = e->n;
    if (n_reads) *n_reads = e->n_reads;
    return 0;
}
void ba_seeding_destroy(BaSeeding* e) { delete e; }

// The hand-off: a BaChaining over the seeder's hits where they lie. hit_first is the only thing downloaded; the per-anchor conditions of
// chaining_plan hold by construction (hit_len = k >= 4, sorted by (r_hit, q_hit), every hit inside sequences shorter than 2^31 - 16).
BaChaining* ba_chaining_create_seeded(const BaChainingParams* params, BaSeeding* s) {
    if (!params) { fail("null argument"); return nullptr; }
    if (!s) { fail("null batch"); return nullptr; }
    if (chaining_check_params(*params)) return nullptr;
    if (!s->ran) { fail("ba_seeding_run has not been called"); return nullptr; }
    if (hipSetDevice(s->device) != hipSuccess) { fail("hipSetDevice failed"); return nullptr; }
    const size_t n = s->n;
    std::vector<uint64_t> first(n + 1);
    if (d2h(s->hit_first, first.data(), n + 1)) return nullptr;
    for (size_t p = 0; p < n; p++) {
        const uint64_t sum = (first[p + 1] - first[p]) * s->P.k;
        if (sum * (uint64_t)params->match_w >= (1ull << 31)) {
            fail("problem %zu: match_w * the sum of anchor_len must stay below 2^31 (it is %llu)", p, (unsigned long long)(sum * (uint64_t)params->match_w));
            return nullptr;
        }
    }
    std::vector<uint32_t> order(n);
    for (size_t p = 0; p < n; p++) order[p] = (uint32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first[a + 1] - first[a] > first[b + 1] - first[b]; });
    std::unique_ptr<BaChaining> e(new BaChaining);
    e->device = s->device; e->P = *params;
    e->ring = 128;
    while (e->ring < params->lookback + 64u) e->ring <<= 1;
    // (a seeder over a multi-sequence index: its hits are in that index's frame and each lies inside one sequence, so the chainer is bounded)
    if (e->open(4) || (s->index && s->index->multi && chaining_bound(e.get(), s->index->seq_start)) ||
        chaining_load(e.get(), first.data(), s->q_hit.as<uint32_t>(), s->r_hit.as<uint32_t>(), s->hit_len.as<uint32_t>(), n, order, true,
                      hipMemcpyDeviceToDevice)) return nullptr;
    return e.release();
}

// ------------------------------------------------------------------ read-level selection (ba_select_*)
// From candidates in any order to the marks of a mapper's records (ba_select.hip; the rule: INTEGRATION.md, "Selecting a read's
// alignments"). The host checks the arguments and orders the reads by their number of candidates; the grouping, the marking and the emit
// are the device's. A selection is small work over many candidates, so what a call costs besides its kernels is kept to a few driver
// calls: every array of a selector lies in ONE device allocation, the host's inputs go up in one copy and the outputs come back in one.
static_assert(sizeof(BaSelectParams) == 24, "struct BaSelectParams is six 4-byte fields");
// Byte offsets in that allocation for a capacity of n candidates and r reads, every array 16-byte aligned: the inputs that always come from
// the host (0 .. in_b), the scores and spans (in_b .. in_end: from the host, or device to device from a chain batch), the scratch, and the
// outputs (out .. out_end). kept has room for every candidate, so no output grows between the passes.
extern "C++" {   // (member templates)
struct SelectLayout {
    size_t read, q_len, support, order, strand, exclude, in_b, score, q_start, q_end, in_end;
    size_t status, a, b, counts, counter, first, keys;   // counts: per read the count, then (r entries on) the scatter's cursor
    size_t out, kept_first, parent, rank, sub_score, n_kept, kept, cls, mapq, out_end;
    explicit SelectLayout(size_t n = 0, size_t r = 0) {
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15) & ~(size_t)15; return o; };
        read = take(n * 4); q_len = take(n * 4); support = take(n * 4); order = take(r * 4); strand = take(n); exclude = take(n);
        in_b = score = take(n * 4); q_start = take(n * 4); q_end = take(n * 4);
        in_end = status = take(n * 4); a = take(n * 4); b = take(n * 4); counts = take(2 * r * 4); counter = take(4); first = take((r + 1) * 8); keys = take(n * 8);
        out = kept_first = take((r + 1) * 8); parent = take(n * 4); rank = take(n * 4); sub_score = take(n * 4); n_kept = take(r * 4); kept = take(n * 4);
        cls = take(n); mapq = take(n);
        out_end = at;
    }
};
// Creating a stream takes milliseconds and a selection a fraction of one, so a selector that is destroyed leaves its stream -- idle: every
// call waits for what it launched -- to the next one on the same device. At most SELECT_STREAMS of them are kept.
constexpr size_t SELECT_STREAMS = 4;
static std::mutex g_select_mutex;
static std::vector<std::pair<int, hipStream_t>> g_select_streams;
struct BaSelect : StreamOwner {
    int open_select(size_t n_events) {   // StreamOwner::open, with a stream that a destroyed selector left if there is one
        {
            std::lock_guard<std::mutex> lock(g_select_mutex);
            for (size_t i = 0; i < g_select_streams.size(); i++)
                if (g_select_streams[i].first == device) { stream = g_select_streams[i].second; g_select_streams.erase(g_select_streams.begin() + i); break; }
        }
        if (!stream) return open(n_events);
        for (size_t i = 0; i < n_events; i++) if (hipEventCreate(&ev[i]) != hipSuccess) return fail("hipEventCreate failed");
        return 0;
    }
    ~BaSelect() {
        std::lock_guard<std::mutex> lock(g_select_mutex);
        if (stream && g_select_streams.size() < SELECT_STREAMS) { g_select_streams.emplace_back(device, stream); stream = nullptr; }
    }
    BaSelectParams P{};
    uint32_t n = 0, n_reads = 0;
    uint64_t cap_n = 0, cap_reads = 0, total_kept = 0;
    bool has_strand = false, has_support = false, has_exclude = false, chained = false, ran = false;
    SelectLayout L;
    DevBuf arena;
    std::vector<uint8_t> stage, mirror;   // the inputs as they go up (0 .. in_end), the outputs as they came back (out .. out_end)
    float group_ms = 0, mark_ms = 0, emit_ms = 0;
    template <class T> T* dev(size_t off) const { return (T*)(arena.as<uint8_t>() + off); }
    template <class T> T* up(size_t off) { return (T*)(stage.data() + off); }
    template <class T> const T* got(size_t off) const { return (const T*)(mirror.data() + (off - L.out)); }
    ba::SelectParams params() const {
        ba::SelectParams sp{};
        sp.n = n; sp.n_reads = n_reads; sp.mask_permille = P.mask_permille; sp.sec_permille = P.sec_permille; sp.max_secondary = P.max_secondary;
        sp.mapq_max = P.mapq_max; sp.full_support = P.full_support; sp.min_score = P.min_score; sp.failed = ba::STATS_FAILED;
        sp.read = dev<uint32_t>(L.read); sp.score = dev<int32_t>(L.score); sp.q_start = dev<uint32_t>(L.q_start); sp.q_end = dev<uint32_t>(L.q_end);
        sp.q_len = dev<uint32_t>(L.q_len); sp.strand = has_strand ? dev<uint8_t>(L.strand) : nullptr; sp.support = has_support ? dev<uint32_t>(L.support) : nullptr;
        sp.exclude = has_exclude ? dev<uint8_t>(L.exclude) : nullptr; sp.status = chained ? dev<uint32_t>(L.status) : nullptr;
        sp.order = dev<uint32_t>(L.order); sp.counter = dev<uint32_t>(L.counter);
        sp.a = dev<uint32_t>(L.a); sp.b = dev<uint32_t>(L.b); sp.count = dev<uint32_t>(L.counts); sp.cursor = dev<uint32_t>(L.counts) + cap_reads;
        sp.first = dev<uint64_t>(L.first); sp.keys = dev<uint64_t>(L.keys);
        sp.cls = dev<uint8_t>(L.cls); sp.mapq = dev<uint8_t>(L.mapq); sp.parent = dev<uint32_t>(L.parent); sp.rank = dev<uint32_t>(L.rank);
        sp.sub_score = dev<int32_t>(L.sub_score); sp.n_kept = dev<uint32_t>(L.n_kept); sp.kept_first = dev<uint64_t>(L.kept_first); sp.kept = dev<uint32_t>(L.kept);
        return sp;
    }
};
template <class T> static void select_get(const BaSelect* e, size_t off, T* dst, size_t count) {   // from the host's image of the outputs
    if (dst && count) memcpy(dst, e->got<T>(off), count * sizeof(T));
}
}  // extern "C++"
static int select_check_params(const BaSelectParams& P) {
    if (P.mask_permille < 1 || P.mask_permille > 1000) return fail("select: mask_permille must be between 1 and 1000 (it is %u)", P.mask_permille);
    if (P.sec_permille > 1000) return fail("select: sec_permille must be between 0 and 1000 (it is %u)", P.sec_permille);
    if (P.mapq_max > 255) return fail("select: mapq_max must be between 0 and 255 (it is %u)", P.mapq_max);
    if (P.full_support < 1 || P.full_support > 65535) return fail("select: full_support must be between 1 and 65535 (it is %u)", P.full_support);
    if (P.min_score < 1) return fail("select: min_score must be at least 1 (it is %d)", P.min_score);
    return 0;
}
// Check a set of candidates (q_start, q_end and q_len null: a chain batch's, which are its own results) -> the reads ordered by their number
// of candidates, the one with the most first.
static int select_plan(const uint32_t* read, const uint32_t* q_start, const uint32_t* q_end, const uint32_t* q_len, const uint8_t* strand, size_t n,
                       size_t n_reads, std::vector<uint32_t>& order) {
    if (n == 0 || n > (1u << 28)) return fail("a selection must hold between 1 and 2^28 candidates");
    if (n_reads == 0 || n_reads > (1u << 28)) return fail("a selection must hold between 1 and 2^28 reads");
    std::vector<uint32_t> per(n_reads, 0);
    for (size_t c = 0; c < n; c++) {
        if (read[c] >= n_reads) return fail("candidate %zu: read %u is not below n_reads (%zu)", c, read[c], n_reads);
        if (q_start && q_start[c] > q_end[c]) return fail("candidate %zu: q_start %u lies behind q_end %u", c, q_start[c], q_end[c]);
        if (q_start && q_end[c] > q_len[c]) return fail("candidate %zu: q_end %u lies behind the end of the read (q_len %u)", c, q_end[c], q_len[c]);
        if (strand && strand[c] > 1) return fail("candidate %zu: strand must be 0 or 1", c);
        if (++per[read[c]] > ba::SELECT_MAX_PER_READ)
            return fail("read %u holds more than %u candidates (candidate %zu is one too many)", read[c], ba::SELECT_MAX_PER_READ, c);
    }
    order.resize(n_reads);
    for (size_t r = 0; r < n_reads; r++) order[r] = (uint32_t)r;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return per[x] > per[y]; });
    return 0;
}
static int select_alloc(BaSelect* e, size_t n, size_t n_reads) {
    e->cap_n = n; e->cap_reads = n_reads;
    e->L = SelectLayout(n, n_reads);
    e->stage.assign(e->L.in_end, 0); e->mirror.assign(e->L.out_end - e->L.out, 0);
    return e->arena.alloc(e->L.out_end);
}
// the inputs that always come from the host, into the staging image (strand, support and exclude may be null)
static void select_stage(BaSelect* e, const uint32_t* read, const uint32_t* q_len, const uint8_t* strand, const uint32_t* support, const uint8_t* exclude,
                         size_t n, const std::vector<uint32_t>& order) {
    memcpy(e->up<uint32_t>(e->L.read), read, n * 4); memcpy(e->up<uint32_t>(e->L.q_len), q_len, n * 4);
    memcpy(e->up<uint32_t>(e->L.order), order.data(), order.size() * 4);
    if (strand) memcpy(e->up<uint8_t>(e->L.strand), strand, n);
    if (support) memcpy(e->up<uint32_t>(e->L.support), support, n * 4);
    if (exclude) memcpy(e->up<uint8_t>(e->L.exclude), exclude, n);
    e->has_strand = strand != nullptr; e->has_support = support != nullptr; e->has_exclude = exclude != nullptr;
}
static int select_load(BaSelect* e, const uint32_t* read, const int32_t* score, const uint32_t* q_start, const uint32_t* q_end, const uint32_t* q_len,
                       const uint8_t* strand, const uint32_t* support, const uint8_t* exclude, size_t n, size_t n_reads, const std::vector<uint32_t>& order,
                       bool create) {
    if (create) { if (select_alloc(e, n, n_reads)) return 1; }
    else if (over_count("candidates", n, e->cap_n) || over_count("reads", n_reads, e->cap_reads)) return 1;
    e->n = 0; e->ran = false;   // (a failure from here on leaves no candidates loaded)
    select_stage(e, read, q_len, strand, support, exclude, n, order);
    memcpy(e->up<int32_t>(e->L.score), score, n * 4); memcpy(e->up<uint32_t>(e->L.q_start), q_start, n * 4); memcpy(e->up<uint32_t>(e->L.q_end), q_end, n * 4);
    HIP_TRY(hipMemcpy(e->arena.p, e->stage.data(), e->L.in_end, hipMemcpyHostToDevice));
    e->n = (uint32_t)n; e->n_reads = (uint32_t)n_reads;
    return 0;
}
BaSelect* ba_select_create(const BaSelectParams* params, const uint32_t* read, const int32_t* score, const uint32_t* q_start, const uint32_t* q_end,
                           const uint32_t* q_len, const uint8_t* strand, const uint32_t* support, const uint8_t* exclude, uintptr_t n, uintptr_t n_reads) {
    std::vector<uint32_t> order;   // every argument is checked before the device is touched
    if (!params || !read || !score || !q_start || !q_end || !q_len) { fail("null argument"); return nullptr; }
    if (select_check_params(*params) || select_plan(read, q_start, q_end, q_len, strand, n, n_reads, order)) return nullptr;
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaSelect> e(new BaSelect);
    e->device = g_device; e->P = *params;
    if (e->open_select(4) || select_load(e.get(), read, score, q_start, q_end, q_len, strand, support, exclude, n, n_reads, order, true)) return nullptr;
    return e.release();
}
// The hand-off: a selector over the results of a chain batch that has run, where they lie. Nothing of the batch's results passes through the
// host; q_len and strand are the host copies the batch keeps for its strings.
BaSelect* ba_select_create_chained(const BaSelectParams* params, BaChainBatch* b, const uint32_t* read_of_chain, const uint32_t* support, uintptr_t n_reads) {
    std::vector<uint32_t> order;
    if (!params) { fail("null argument"); return nullptr; }
    if (!b) { fail("null batch"); return nullptr; }
    if (!read_of_chain) { fail("null argument"); return nullptr; }
    if (select_check_params(*params)) return nullptr;
    if (!b->ran) { fail("select: the batch has not finished a run (ba_chain_batch_run)"); return nullptr; }
    const size_t n = b->n;
    if (select_plan(read_of_chain, nullptr, nullptr, nullptr, nullptr, n, n_reads, order)) return nullptr;
    if (hipSetDevice(b->device) != hipSuccess) { fail("hipSetDevice failed"); return nullptr; }
    std::unique_ptr<BaSelect> e(new BaSelect);
    e->device = b->device; e->P = *params; e->chained = true;
    if (e->open_select(4) || select_alloc(e.get(), n, n_reads)) return nullptr;
    // on the selector's own stream, which its kernels follow, and waited for: the batch may be reloaded or destroyed as soon as this call is over
    const std::pair<size_t, const DevBuf*> copies[] = {{e->L.score, &b->score}, {e->L.q_start, &b->q_start}, {e->L.q_end, &b->q_end}, {e->L.status, &b->status}};
    for (const auto& cp : copies)
        if (hipMemcpyAsync(e->dev<uint8_t>(cp.first), cp.second->p, n * 4, hipMemcpyDeviceToDevice, e->stream) != hipSuccess) { fail("hipMemcpyAsync failed"); return nullptr; }
    select_stage(e.get(), read_of_chain, b->h_t_ql.data(), b->h_t_strand.data(), support, nullptr, n, order);
    if (hipMemcpyAsync(e->arena.p, e->stage.data(), e->L.in_b, hipMemcpyHostToDevice, e->stream) != hipSuccess) { fail("hipMemcpyAsync failed"); return nullptr; }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { fail("hipStreamSynchronize failed"); return nullptr; }
    e->n = (uint32_t)n; e->n_reads = (uint32_t)n_reads;
    return e.release();
}
int ba_select_reload(BaSelect* e, const uint32_t* read, const int32_t* score, const uint32_t* q_start, const uint32_t* q_end, const uint32_t* q_len,
                     const uint8_t* strand, const uint32_t* support, const uint8_t* exclude, uintptr_t n, uintptr_t n_reads) {
    if (!e) return fail("null batch");
    if (e->chained) return fail("reload: the selector reads a chain batch's results (ba_select_create_chained makes another one from a batch that has run)");
    if (!read || !score || !q_start || !q_end || !q_len) return fail("null argument");
    std::vector<uint32_t> order;
    if (select_plan(read, q_start, q_end, q_len, strand, n, n_reads, order)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return select_load(e, read, score, q_start, q_end, q_len, strand, support, exclude, n, n_reads, order, false);
}
int ba_select_run(BaSelect* e, float* kernels_ms) {
    if (!e) return fail("null batch");
    if (!e->n) return fail("no candidates loaded (the last reload failed)");
    HIP_TRY(hipSetDevice(e->device));
    e->ran = false; e->group_ms = e->mark_ms = e->emit_ms = 0; e->total_kept = 0;
    const ba::SelectParams sp = e->params();
    HIP_TRY(hipMemsetAsync(sp.count, 0, 2 * (size_t)e->cap_reads * 4, e->stream));
    HIP_TRY(hipMemsetAsync(sp.counter, 0, 4, e->stream));
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    HIP_TRY(ba_launch_select_group(e->stream, &sp, 0));
    HIP_TRY(ba_launch_offsets(e->stream, sp.count, e->dev<uint64_t>(e->L.first), sp.n_reads));
    HIP_TRY(ba_launch_select_group(e->stream, &sp, 1));
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    HIP_TRY(ba_launch_select_mark(e->stream, &sp));
    HIP_TRY(ba_launch_offsets(e->stream, sp.n_kept, e->dev<uint64_t>(e->L.kept_first), sp.n_reads));
    HIP_TRY(hipEventRecord(e->ev[2], e->stream));
    HIP_TRY(ba_launch_select_emit(e->stream, &sp));   // (kept has room for every candidate: the host need not read the total in between)
    HIP_TRY(hipEventRecord(e->ev[3], e->stream));
    // every output in one copy, on the stream behind the kernels; the getters read the host's image
    HIP_TRY(hipMemcpyAsync(e->mirror.data(), e->dev<uint8_t>(e->L.out), e->L.out_end - e->L.out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->elapsed(0, 1, &e->group_ms) || e->elapsed(1, 2, &e->mark_ms) || e->elapsed(2, 3, &e->emit_ms)) return 1;
    const uint64_t kept = e->got<uint64_t>(e->L.kept_first)[e->n_reads];
    if (kept > e->n) return fail("select: the device kept %llu candidates, more than the set holds", (unsigned long long)kept);
    e->total_kept = kept;
    e->ran = true;
    if (kernels_ms) *kernels_ms = e->group_ms + e->mark_ms + e->emit_ms;
    return 0;
}
int ba_select_counts(BaSelect* e, uint64_t* n_kept, uint32_t* kept_per_read) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_select_run has not been called");
    if (n_kept) *n_kept = e->total_kept;
    select_get(e, e->L.n_kept, kept_per_read, e->n_reads);
    return 0;
}
int ba_select_results(BaSelect* e, uint8_t* cls, uint8_t* mapq, uint32_t* parent, uint32_t* rank, int32_t* sub_score) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_select_run has not been called");
    select_get(e, e->L.cls, cls, e->n); select_get(e, e->L.mapq, mapq, e->n); select_get(e, e->L.parent, parent, e->n);
    select_get(e, e->L.rank, rank, e->n); select_get(e, e->L.sub_score, sub_score, e->n);
    return 0;
}
int ba_select_kept(BaSelect* e, uint64_t* kept_first, uint32_t* kept) {
    if (!e) return fail("null batch");
    if (!e->ran) return fail("ba_select_run has not been called");
    select_get(e, e->L.kept_first, kept_first, (size_t)e->n_reads + 1); select_get(e, e->L.kept, kept, e->total_kept);
    return 0;
}
int ba_select_times(BaSelect* e, float* group_ms, float* mark_ms, float* emit_ms) {
    if (!e) return fail("null batch");
    if (group_ms) *group_ms = e->group_ms;
    if (mark_ms) *mark_ms = e->mark_ms;
    if (emit_ms) *emit_ms = e->emit_ms;
    return 0;
}
void ba_select_destroy(BaSelect* e) { delete e; }

// ------------------------------------------------------------------ the reference index (ba_ref_index_*, ba_seeding_*_indexed)
// One reference's sketch, built once, and seeders whose problems are reads against all of it (ba_index.hip; the rule: INTEGRATION.md,
// "Reference index"). The build keeps the reference's bytes on the device only until the keys are written.
struct BaRefIndex {
    std::shared_ptr<IndexData> d;
    float sketch_ms = 0, sort_ms = 0, table_ms = 0;
};
// ref: the bytes of D.seq_start's sequences, laid end to end
static int index_build(BaRefIndex* x, const uint8_t* ref) {
    IndexData& D = *x->d;
    const uint32_t len = (uint32_t)D.ref_len, k = D.k, w = D.w;
    const size_t n_seqs = D.seq_start.size() - 1;
    // the work items: a sequence's windows in spans of INDEX_SPAN, numbered from seq_span[s] (a sequence without a k-mer has no window)
    std::vector<uint64_t> seq_span(n_seqs + 1, 0);
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t sl = D.seq_start[s + 1] - D.seq_start[s], nk = sl >= k ? sl - k + 1u : 0u, nw = nk == 0u ? 0u : nk > w ? nk - w + 1u : 1u;
        seq_span[s + 1] = seq_span[s] + (nw + ba::INDEX_SPAN - 1u) / ba::INDEX_SPAN;
    }
    StreamOwner T;   // the stream and the six events of this build (made below with the build's own error texts, destroyed with T)
    DevBuf raw, counter, span_cnt, span_first, unsorted, temp, longest, d_seq_start, d_seq_span;
    ba::IndexParams ip{};
    ip.k = k; ip.w = w; ip.len = len; ip.n_seqs = (uint32_t)n_seqs; ip.n_spans = (uint32_t)seq_span[n_seqs]; ip.prefix_bits = D.prefix_bits;
    HIP_TRY(hipStreamCreateWithFlags(&T.stream, hipStreamNonBlocking));
    for (int i = 0; i < 6; i++) HIP_TRY(hipEventCreate(&T.ev[i]));
    if (raw.alloc(len) || counter.alloc(4) || span_cnt.alloc((size_t)ip.n_spans * 4) || span_first.alloc(((size_t)ip.n_spans + 1) * 8) || longest.alloc(4) ||
        D.table.alloc(((size_t)(1u << ip.prefix_bits) + 1) * 4) || d_seq_start.alloc((n_seqs + 1) * 8) || d_seq_span.alloc((n_seqs + 1) * 8)) return 1;
    if (len && h2d(raw, ref, len)) return 1;
    if (h2d(d_seq_start, D.seq_start.data(), n_seqs + 1) || h2d(d_seq_span, seq_span.data(), n_seqs + 1)) return 1;
    ip.ref = raw.as<uint8_t>(); ip.counter = counter.as<uint32_t>(); ip.span_cnt = span_cnt.as<uint32_t>(); ip.span_first = span_first.as<uint64_t>();
    ip.seq_start = d_seq_start.as<uint64_t>(); ip.seq_span = d_seq_span.as<uint64_t>();
    ip.table = D.table.as<uint32_t>(); ip.longest_run = longest.as<uint32_t>();
    // the sketch: count, scan, emit
    HIP_TRY(hipMemsetAsync(counter.p, 0, 4, T.stream));
    HIP_TRY(hipEventRecord(T.ev[0], T.stream));
    HIP_TRY(D.canonical ? ba_launch_both_index_sketch(T.stream, &ip, 0) : ba_launch_index_sketch(T.stream, &ip, 0));
    HIP_TRY(ba_launch_offsets(T.stream, ip.span_cnt, span_first.as<uint64_t>(), ip.n_spans));
    HIP_TRY(hipEventRecord(T.ev[1], T.stream));
    HIP_TRY(hipStreamSynchronize(T.stream));
    uint64_t total = 0;
    HIP_TRY(hipMemcpy(&total, span_first.as<uint64_t>() + ip.n_spans, 8, hipMemcpyDeviceToHost));
    if (unsorted.alloc(total * 8) || D.key.alloc(total * 8)) return 1;
    ip.n_entries = (uint32_t)total; ip.unsorted = unsorted.as<uint64_t>(); ip.key = D.key.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(counter.p, 0, 4, T.stream));
    HIP_TRY(hipEventRecord(T.ev[2], T.stream));
    HIP_TRY(D.canonical ? ba_launch_both_index_sketch(T.stream, &ip, 1) : ba_launch_index_sketch(T.stream, &ip, 1));
    HIP_TRY(hipEventRecord(T.ev[3], T.stream));
    // the sort of the keys (a code has 2k bits above the position's 32), the table
    if (total) {
        size_t temp_bytes = 0;
        HIP_TRY(ba_launch_index_sort(T.stream, ip.unsorted, D.key.as<uint64_t>(), ip.n_entries, 32u + 2u * k, nullptr, &temp_bytes));
        if (temp.alloc(temp_bytes)) return 1;
        HIP_TRY(ba_launch_index_sort(T.stream, ip.unsorted, D.key.as<uint64_t>(), ip.n_entries, 32u + 2u * k, temp.p, &temp_bytes));
    }
    HIP_TRY(hipEventRecord(T.ev[4], T.stream));
    HIP_TRY(hipMemsetAsync(longest.p, 0, 4, T.stream));
    HIP_TRY(ba_launch_index_table(T.stream, &ip));
    HIP_TRY(hipEventRecord(T.ev[5], T.stream));
    HIP_TRY(hipStreamSynchronize(T.stream));
    HIP_TRY(hipMemcpy(&D.longest_run, longest.p, 4, hipMemcpyDeviceToHost));
    D.n_entries = total;
    float a = 0, b = 0;
    if (T.elapsed(0, 1, &a) || T.elapsed(2, 3, &b)) return 1;
    x->sketch_ms = a + b;
    return T.elapsed(3, 4, &x->sort_ms) || T.elapsed(4, 5, &x->table_ms);
}
// An index over the sequences that start (one entry more than sequences) lays end to end in ref.
static BaRefIndex* index_create(uint32_t k, uint32_t w, const uint8_t* ref, std::vector<uint64_t> start, bool multi, bool canonical) {
    if (ensure_device()) return nullptr;
    std::unique_ptr<BaRefIndex> x(new BaRefIndex);
    x->d = std::make_shared<IndexData>();
    x->d->device = g_device; x->d->k = k; x->d->w = w; x->d->ref_len = start.back();
    x->d->seq_start = std::move(start); x->d->multi = multi; x->d->canonical = canonical;
    x->d->prefix_bits = 2u * k < ba::INDEX_MAX_PREFIX_BITS ? 2u * k : ba::INDEX_MAX_PREFIX_BITS;
    if (index_build(x.get(), ref)) return nullptr;
    return x.release();
}
BaRefIndex* ba_ref_index_create(uint32_t k, uint32_t w, const uint8_t* ref, uint64_t ref_len) {
    if (seeding_check_params(BaSeedingParams{k, w, 1})) return nullptr;   // every argument is checked before the device is touched
    if (!ref) { fail("null argument"); return nullptr; }
    if (ref_len >= ba::SEEDING_MAX_LEN) { fail("the reference (%llu bytes) must be shorter than 2^31 - 16 bytes", (unsigned long long)ref_len); return nullptr; }
    return index_create(k, w, ref, {0, ref_len}, false, false);   // (one sequence, read where it lies)
}
// Several sequences in one index ("Several sequences"): pool[seq_off[s] .. + seq_len[s]), laid end to end without a spacer.
static BaRefIndex* index_create_seqs(uint32_t k, uint32_t w, const uint8_t* pool, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs, bool canonical) {
    if (seeding_check_params(BaSeedingParams{k, w, 1})) return nullptr;   // every argument is checked before the device is touched
    if (!pool || !seq_off || !seq_len) { fail("null argument"); return nullptr; }
    std::vector<uint64_t> start;
    if (seq_table_from_len(seq_len, n_seqs, start)) return nullptr;
    std::vector<uint8_t> bytes(start[n_seqs]);   // (one upload, whatever the number of sequences and wherever they lie in the pool)
    for (size_t s = 0; s < n_seqs; s++)
        if (seq_len[s]) memcpy(bytes.data() + start[s], pool + seq_off[s], seq_len[s]);
    return index_create(k, w, bytes.data(), std::move(start), true, canonical);
}
BaRefIndex* ba_ref_index_create_multi(uint32_t k, uint32_t w, const uint8_t* pool, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs) {
    return index_create_seqs(k, w, pool, seq_off, seq_len, n_seqs, false);
}
// The same over canonical k-mers ("Both strands at once"): what ba_seeding_create_indexed_both seeds against.
BaRefIndex* ba_ref_index_create_canonical(uint32_t k, uint32_t w, const uint8_t* pool, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs) {
    return index_create_seqs(k, w, pool, seq_off, seq_len, n_seqs, true);
}
int ba_ref_index_is_canonical(BaRefIndex* x, int* flag) {
    if (!x) return fail("null index");
    if (flag) *flag = x->d->canonical ? 1 : 0;
    return 0;
}
int ba_ref_index_sequences(BaRefIndex* x, uint64_t* n_seqs, uint64_t* seq_start) {
    if (!x) return fail("null index");
    if (n_seqs) *n_seqs = x->d->seq_start.size() - 1;
    if (seq_start) std::copy(x->d->seq_start.begin(), x->d->seq_start.end(), seq_start);
    return 0;
}
int ba_ref_index_counts(BaRefIndex* x, uint64_t* n_entries, uint32_t* k, uint32_t* w, uint64_t* ref_len, uint32_t* longest_run) {
    if (!x) return fail("null index");
    if (n_entries) *n_entries = x->d->n_entries;
    if (k) *k = x->d->k;
    if (w) *w = x->d->w;
    if (ref_len) *ref_len = x->d->ref_len;
    if (longest_run) *longest_run = x->d->longest_run;
    return 0;
}
int ba_ref_index_entries(BaRefIndex* x, uint32_t* code, uint32_t* pos) {
    if (!x) return fail("null index");
    HIP_TRY(hipSetDevice(x->d->device));
    std::vector<uint64_t> key(x->d->n_entries);
    if (d2h(x->d->key, key.data(), key.size())) return 1;
    for (size_t i = 0; i < key.size(); i++) {
        if (code) code[i] = (uint32_t)(key[i] >> 32);
        if (pos) pos[i] = (uint32_t)key[i];
    }
    return 0;
}
int ba_ref_index_times(BaRefIndex* x, float* sketch_ms, float* sort_ms, float* table_ms) {
    if (!x) return fail("null index");
    if (sketch_ms) *sketch_ms = x->sketch_ms;
    if (sort_ms) *sort_ms = x->sort_ms;
    if (table_ms) *table_ms = x->table_ms;
    return 0;
}
void ba_ref_index_destroy(BaRefIndex* x) { delete x; }

// (The index is looked at last: the other arguments are judged without one, so without a device as well.)
BaSeeding* ba_seeding_create_indexed(BaRefIndex* x, uint32_t max_occ, uint32_t max_ref_occ, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len,
                                     const uint8_t* strand, uintptr_t n_problems) {
    SeedingSet S;
    if (max_occ < 1) { fail("seeding: max_occ must be at least 1"); return nullptr; }
    if (max_ref_occ < 1) { fail("seeding: max_ref_occ must be at least 1"); return nullptr; }
    if (seeding_plan(pool, q_off, q_len, nullptr, nullptr, strand, n_problems, S, true)) return nullptr;   // (empty references: the sketch skips them)
    if (!x) { fail("null index"); return nullptr; }
    if (x->d->canonical) { fail("ba_seeding_create_indexed: the index is canonical and holds both strands; call ba_seeding_create_indexed_both"); return nullptr; }
    if (hipSetDevice(x->d->device) != hipSuccess) { fail("hipSetDevice failed"); return nullptr; }   // the seeder lives on the index's device
    std::unique_ptr<BaSeeding> e(new BaSeeding);
    e->device = x->d->device; e->P = BaSeedingParams{x->d->k, x->d->w, max_occ};
    e->index = x->d; e->max_ref_occ = max_ref_occ;
    if (e->open(9) || seeding_load(e.get(), S, true)) return nullptr;
    return e.release();
}
int ba_seeding_reload_indexed(BaSeeding* e, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint8_t* strand, uintptr_t n_problems) {
    if (!e) return fail("null batch");
    if (e->both) return fail("ba_seeding_reload_indexed: the seeder takes its reads on both strands at once; call ba_seeding_reload_indexed_both");
    if (!e->index) return fail("ba_seeding_reload_indexed: the seeder was created without a reference index; call ba_seeding_reload");
    SeedingSet S;
    if (seeding_plan(pool, q_off, q_len, nullptr, nullptr, strand, n_problems, S, true)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return seeding_load(e, S, false);
}

// ------------------------------------------------------------------ both strands at once (ba_seeding_*_indexed_both)
// n reads against a canonical index, each sketched once: read r on strand s is problem 2 r + s of a BaSeeding with 2 n problems
// (ba_index_both.hip; the rule: INTEGRATION.md, "Both strands at once"). Such a seeder is a set with other counts (seeding_plan_both) and
// two kernels of its own; seeding_load loads it and ba_seeding_run runs it, in the seeding section above.
static int seeding_plan_both(const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, size_t n_reads, SeedingSet& S) {
    if (!pool || !q_off || !q_len) return fail("null argument");
    if (n_reads == 0 || n_reads > (1u << 27)) return fail("a both-strand seeding batch must hold between 1 and 2^27 reads");
    for (size_t r = 0; r < n_reads; r++)   // (seeding_plan checks the lengths again: this loop is here for the wording, reads and not problems)
        if (q_len[r] >= ba::SEEDING_MAX_LEN) return fail("read %zu: the read (%u bytes) must be shorter than 2^31 - 16 bytes", r, q_len[r]);
    if (seeding_plan(pool, q_off, q_len, nullptr, nullptr, nullptr, n_reads, S, true)) return 1;
    // the reads are all that is sketched, in the order of the sort, and none has a strand; two problems each
    S.n_seqs = n_reads; S.n_match = S.n_problems = 2 * n_reads; S.nouns = "reads";
    S.off.resize(n_reads); S.len.resize(n_reads); S.rc.clear(); S.seq_order.clear();
    S.match_order.resize(2 * n_reads);   // the problems for the sort of the hits: both of a read, the reads longest first
    for (size_t t = 0; t < n_reads; t++) { S.match_order[2 * t] = 2 * S.sort_order[t]; S.match_order[2 * t + 1] = 2 * S.sort_order[t] + 1; }
    return 0;
}
BaSeeding* ba_seeding_create_indexed_both(BaRefIndex* x, uint32_t max_occ, uint32_t max_ref_occ, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len,
                                          uintptr_t n_reads) {
    SeedingSet S;   // (the index is looked at last, as in ba_seeding_create_indexed)
    if (max_occ < 1) { fail("seeding: max_occ must be at least 1"); return nullptr; }
    if (max_ref_occ < 1) { fail("seeding: max_ref_occ must be at least 1"); return nullptr; }
    if (seeding_plan_both(pool, q_off, q_len, n_reads, S)) return nullptr;
    if (!x) { fail("null index"); return nullptr; }
    if (!x->d->canonical) {
        fail("ba_seeding_create_indexed_both: the index is not canonical (ba_ref_index_create_canonical makes one); call ba_seeding_create_indexed");
        return nullptr;
    }
    if (hipSetDevice(x->d->device) != hipSuccess) { fail("hipSetDevice failed"); return nullptr; }   // the seeder lives on the index's device
    std::unique_ptr<BaSeeding> e(new BaSeeding);
    e->device = x->d->device; e->P = BaSeedingParams{x->d->k, x->d->w, max_occ};
    e->index = x->d; e->max_ref_occ = max_ref_occ; e->both = true;
    if (e->open(9) || seeding_load(e.get(), S, true)) return nullptr;
    return e.release();
}
int ba_seeding_reload_indexed_both(BaSeeding* e, const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n_reads) {
    if (!e) return fail("null batch");
    if (!e->both) return fail("ba_seeding_reload_indexed_both: the seeder takes one strand per problem; call %s", e->index ? "ba_seeding_reload_indexed" : "ba_seeding_reload");
    SeedingSet S;
    if (seeding_plan_both(pool, q_off, q_len, n_reads, S)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return seeding_load(e, S, false);
}
// Candidate windows for chain batches: the reference stretch a chain can reach, so that a chain batch over a long reference packs no
// more than that (host only). All arithmetic is 64-bit.
int ba_chain_windows(const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, const uint64_t* anchor_first, const uint32_t* q_anchor,
                     const uint32_t* r_anchor, const uint32_t* anchor_len, uintptr_t n_chains, uint32_t margin, uint64_t* r_off_out, uint32_t* r_len_out,
                     uint32_t* r_anchor_out) {
    if (!q_len || !r_off || !r_len || !anchor_first || !q_anchor || !r_anchor || !anchor_len || !r_off_out || !r_len_out || !r_anchor_out) return fail("null argument");
    for (size_t c = 0; c < n_chains; c++) {
        const uint64_t a0 = anchor_first[c], a1 = anchor_first[c + 1];
        if (a1 <= a0) return fail("chain %zu has no anchors", c);
        for (uint64_t a = a0; a < a1; a++)
            if ((uint64_t)q_anchor[a] + anchor_len[a] > q_len[c] || (uint64_t)r_anchor[a] + anchor_len[a] > r_len[c])
                return fail("chain %zu: anchor %llu ends outside its sequences", c, (unsigned long long)(a - a0));
        const uint64_t qa0 = q_anchor[a0], ra0 = r_anchor[a0], qe = (uint64_t)q_anchor[a1 - 1] + anchor_len[a1 - 1], re = (uint64_t)r_anchor[a1 - 1] + anchor_len[a1 - 1];
        const uint64_t lo = ra0 - std::min(ra0, qa0 + margin), hi = re + std::min(r_len[c] - re, (q_len[c] - qe) + margin);
        r_off_out[c] = r_off[c] + lo;
        r_len_out[c] = (uint32_t)(hi - lo);
        for (uint64_t a = a0; a < a1; a++) r_anchor_out[a] = (uint32_t)(r_anchor[a] - lo);
    }
    return 0;
}
// The same for chains in the frame of a multi-sequence index ("Several sequences"): a window stays inside the sequence that holds the
// chain's first anchor, and comes out as bytes of the caller's pool, where only seq_off says where a sequence lies (host only).
int ba_chain_windows_seqs(const uint32_t* q_len, const uint64_t* anchor_first, const uint32_t* q_anchor, const uint32_t* r_anchor, const uint32_t* anchor_len,
                          uintptr_t n_chains, uint32_t margin, const uint64_t* seq_off, const uint32_t* seq_len, uintptr_t n_seqs, uint64_t* r_off_out,
                          uint32_t* r_len_out, uint32_t* r_anchor_out, uint32_t* seq_of_chain, uint32_t* local_shift) {
    if (!q_len || !anchor_first || !q_anchor || !r_anchor || !anchor_len || !seq_off || !seq_len || !r_off_out || !r_len_out || !r_anchor_out || !seq_of_chain ||
        !local_shift) return fail("null argument");
    std::vector<uint64_t> start;
    if (seq_table_from_len(seq_len, n_seqs, start)) return 1;
    const SeqTable T(start.data(), n_seqs);
    for (size_t c = 0; c < n_chains; c++) {
        const uint64_t a0 = anchor_first[c], a1 = anchor_first[c + 1];
        if (a1 <= a0) return fail("chain %zu has no anchors", c);
        const size_t s = T.of(r_anchor[a0]);
        const uint64_t S = start[s], E = start[s + 1];
        for (uint64_t a = a0; a < a1; a++)
            if ((uint64_t)q_anchor[a] + anchor_len[a] > q_len[c] || (uint64_t)r_anchor[a] + anchor_len[a] > E)
                return fail("chain %zu: anchor %llu ends outside its sequences", c, (unsigned long long)(a - a0));
        const uint64_t qa0 = q_anchor[a0], ra0 = r_anchor[a0], qe = (uint64_t)q_anchor[a1 - 1] + anchor_len[a1 - 1], re = (uint64_t)r_anchor[a1 - 1] + anchor_len[a1 - 1];
        const uint64_t lo = ra0 - std::min(ra0 - S, qa0 + margin), hi = re + std::min(E - re, (q_len[c] - qe) + margin);
        r_off_out[c] = seq_off[s] + (lo - S);
        r_len_out[c] = (uint32_t)(hi - lo);
        seq_of_chain[c] = (uint32_t)s;
        local_shift[c] = (uint32_t)(lo - S);
        for (uint64_t a = a0; a < a1; a++) r_anchor_out[a] = (uint32_t)(r_anchor[a] - lo);
    }
    return 0;
}
// From the frame of a multi-sequence index to a sequence and positions in it, for closed intervals [r_start, r_end] (host only).
int ba_ref_locate(const uint32_t* seq_len, uintptr_t n_seqs, const uint32_t* r_start, const uint32_t* r_end, uintptr_t n, uint32_t* seq, uint32_t* local_start,
                  uint32_t* local_end, uint8_t* crosses) {
    if (!seq_len || !r_start || !r_end || !seq || !local_start || !local_end || !crosses) return fail("null argument");
    std::vector<uint64_t> start;
    if (seq_table_from_len(seq_len, n_seqs, start)) return 1;
    const SeqTable T(start.data(), n_seqs);
    for (size_t i = 0; i < n; i++) {
        if (r_end[i] < r_start[i] || r_end[i] > T.total())
            return fail("interval %zu: %u to %u is not an interval of the index's %llu bytes", i, r_start[i], r_end[i], (unsigned long long)T.total());
        const size_t s = T.of(r_start[i]);
        seq[i] = (uint32_t)s;
        local_start[i] = (uint32_t)(r_start[i] - start[s]);
        local_end[i] = (uint32_t)(r_end[i] - start[s]);
        crosses[i] = r_end[i] > start[s + 1];
    }
    return 0;
}

int block_batch_align(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                      const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n,
                      AlignResult* results, uint32_t* cigar_runs, uint64_t cigar_capacity, uint32_t* cigar_len) {
    std::unique_ptr<BaBatch> b(ba_batch_create(kind, matrix, gaps, size, x_drop, mode, pool, q_off, q_len, r_off, r_len, n));
    if (!b) return 1;
    if (ba_batch_run(b.get(), nullptr)) return 1;
    std::vector<int32_t> sc(n); std::vector<uint32_t> qi(n), ri(n), st(n);
    if (ba_batch_results(b.get(), sc.data(), qi.data(), ri.data(), nullptr, cigar_len, st.data())) return 1;
    for (size_t p = 0; p < n; p++) {
        if (st[p]) return fail("pair %zu failed on the device (status 0x%x)", p, st[p]);
        if (results) results[p] = AlignResult{sc[p], qi[p], ri[p]};
    }
    if ((mode & BA_TRACE) && cigar_runs) return ba_batch_cigars(b.get(), cigar_runs, cigar_capacity);
    return 0;
}

// ------------------------------------------------------------------ nucleotide / byte objects
NucMatrix* block_new_simple_nucmatrix(int8_t match_score, int8_t mismatch_score) { return new NucMatrix(nuc_simple(match_score, mismatch_score)); }
void block_set_nucmatrix(NucMatrix* m, uint8_t a, uint8_t b, int8_t score) {   // scores.rs:174-183
    a = upper(a); b = upper(b);
    if (!(a >= 'A' && a <= 'Z' && b >= 'A' && b <= 'Z')) die("NucMatrix::set: bytes must be in 'A'..='Z'");
    m->scores[(a & 7) * 16 + (b & 15)] = score;
    m->scores[(b & 7) * 16 + (a & 15)] = score;
}
void block_free_nucmatrix(NucMatrix* m) { delete m; }

static PaddedBytes* padded_new(int kind, size_t len, size_t max_size) {   // scan_block.rs:1798-1803
    PaddedBytes* p = new PaddedBytes;
    p->s.assign(1 + len + max_size, null_byte(kind));
    p->len = len; p->kind = kind;
    return p;
}
static void padded_set(PaddedBytes* p, const uint8_t* s, size_t len, size_t max_size, bool rev) {   // scan_block.rs:1806-1822
    if (1 + len + max_size > p->s.size()) die("PaddedBytes::set_bytes: %zu bytes + %zu padding exceed the allocated %zu", len, max_size, p->s.size());
    p->s[0] = null_byte(p->kind);
    for (size_t k = 0; k < len; k++) {
        uint8_t c;
        if (!convert_char(p->kind, s[rev ? len - 1 - k : k], &c)) die("byte 0x%02x is outside the matrix alphabet", s[rev ? len - 1 - k : k]);
        p->s[1 + k] = c;
    }
    std::fill(p->s.begin() + 1 + len, p->s.begin() + 1 + len + max_size, null_byte(p->kind));
    p->len = len;
}
PaddedBytes* block_new_padded_nuc(uintptr_t len, uintptr_t max_size) { return padded_new(BA_KIND_NUC, len, max_size); }
void block_set_bytes_padded_nuc(PaddedBytes* p, const uint8_t* s, uintptr_t len, uintptr_t max_size) { padded_set(p, s, len, max_size, false); }
void block_set_bytes_rev_padded_nuc(PaddedBytes* p, const uint8_t* s, uintptr_t len, uintptr_t max_size) { padded_set(p, s, len, max_size, true); }
void block_free_padded_nuc(PaddedBytes* p) { delete p; }
PaddedBytes* block_new_padded_bytes(uintptr_t len, uintptr_t max_size) { return padded_new(BA_KIND_BYTES, len, max_size); }
void block_set_bytes_padded_bytes(PaddedBytes* p, const uint8_t* s, uintptr_t len, uintptr_t max_size) { padded_set(p, s, len, max_size, false); }
void block_free_padded_bytes(PaddedBytes* p) { delete p; }

// ------------------------------------------------------------------ Part 1: AAMatrix, PaddedBytes (aa), Cigar
AAMatrix* block_new_simple_aamatrix(int8_t match_score, int8_t mismatch_score) {   // scores.rs:48-61
    AAMatrix* m = new AAMatrix;
    memset(m->scores, 0x80, sizeof m->scores);
    for (int i = 0; i < 26; i++)
        for (int j = 0; j < 26; j++) m->scores[i * 32 + j] = i == j ? match_score : mismatch_score;
    return m;
}
void block_set_aamatrix(AAMatrix* m, uint8_t a, uint8_t b, int8_t score) {   // scores.rs:89-98
    a = upper(a); b = upper(b);
    if (!(a >= 'A' && a <= 'Z' + 1 && b >= 'A' && b <= 'Z' + 1)) die("AAMatrix::set: bytes must be in 'A'..='['");
    m->scores[(a - 'A') * 32 + (b - 'A')] = score;
    m->scores[(b - 'A') * 32 + (a - 'A')] = score;
}
void block_free_aamatrix(AAMatrix* m) { delete m; }

PaddedBytes* block_new_padded_aa(uintptr_t len, uintptr_t max_size) { return padded_new(BA_KIND_AA, len, max_size); }
void block_set_bytes_padded_aa(PaddedBytes* p, const uint8_t* s, uintptr_t len, uintptr_t max_size) { padded_set(p, s, len, max_size, false); }
void block_set_bytes_rev_padded_aa(PaddedBytes* p, const uint8_t* s, uintptr_t len, uintptr_t max_size) { padded_set(p, s, len, max_size, true); }
void block_free_padded_aa(PaddedBytes* p) { delete p; }

Cigar* block_new_cigar(uintptr_t query_len, uintptr_t reference_len) {   // cigar.rs:49-54
    Cigar* c = new Cigar;
    c->capacity = query_len + reference_len + 5;
    return c;
}
OpLen block_get_cigar(const Cigar* c, uintptr_t i) {   // cigar.rs:92-94 (i-th run from the start of the alignment)
    if (i >= c->ops.size()) die("Cigar::get: index %zu out of range (%zu runs)", (size_t)i, c->ops.size());
    return c->ops[i];
}
uintptr_t block_len_cigar(const Cigar* c) { return c->ops.size(); }
void block_free_cigar(Cigar* c) { delete c; }

// ------------------------------------------------------------------ Part 1: AAProfile (host object; scores.rs:470-715)
AAProfile* block_new_aaprofile(uintptr_t str_len, uintptr_t block_size, int8_t gap_extend) {
    AAProfile* p = new AAProfile;
    p->max_len = p->curr_len = str_len + block_size + 1;
    p->str_len = str_len; p->gap_extend = gap_extend;
    p->pos_aa.assign(p->max_len * 32, (int8_t)-128);
    p->gap_open_C.assign(p->max_len, -128); p->gap_close_C.assign(p->max_len, -128); p->gap_open_R.assign(p->max_len, -128);
    return p;
}
uintptr_t block_len_aaprofile(const AAProfile* p) { return p->str_len; }
void block_clear_aaprofile(AAProfile* p, uintptr_t str_len, uintptr_t block_size) {
    const size_t cl = str_len + block_size + 1;
    if (cl > p->max_len) die("AAProfile::clear: length exceeds the allocation");
    std::fill(p->pos_aa.begin(), p->pos_aa.begin() + cl * 32, (int8_t)-128);
    std::fill(p->gap_open_C.begin(), p->gap_open_C.begin() + cl, (int16_t)-128);
    std::fill(p->gap_close_C.begin(), p->gap_close_C.begin() + cl, (int16_t)-128);
    std::fill(p->gap_open_R.begin(), p->gap_open_R.begin() + cl, (int16_t)-128);
    p->str_len = str_len; p->curr_len = cl;
}
void block_set_aaprofile(AAProfile* p, uintptr_t i, uint8_t b, int8_t score) {
    b = upper(b);
    if (!(b >= 'A' && b <= 'Z' + 1)) die("AAProfile::set: byte must be in 'A'..='['");
    if (i >= p->curr_len) die("AAProfile::set: position out of range");
    p->pos_aa[i * 32 + (b - 'A')] = score;
}
static void profile_set_all(AAProfile* p, const uint8_t* order, size_t order_len, const int8_t* scores, size_t scores_len,
                            size_t left_shift, size_t right_shift, bool rev) {   // scores.rs:677-714
    if (order_len == 0 || order_len > 32) die("AAProfile::set_all: order length must be in 1..=32");
    uint8_t o[32];
    for (size_t k = 0; k < order_len; k++) {
        const uint8_t b = upper(order[k]);
        if (!(b >= 'A' && b <= 'Z' + 1)) die("AAProfile::set_all: order byte out of range");
        o[k] = (uint8_t)(b - 'A');
    }
    if (scores_len / order_len != p->str_len) die("AAProfile::set_all: scores length does not match the profile length");
    size_t idx = 0;
    for (size_t n = 0; n < p->str_len; n++) {
        const size_t i = rev ? p->str_len - n : 1 + n;
        for (size_t j = 0; j < order_len; j++) {
            const int8_t sc = (int8_t)((int8_t)((uint8_t)scores[idx] << left_shift) >> right_shift);
            p->pos_aa[i * 32 + o[j]] = sc;
            idx++;
        }
    }
}
void block_set_all_aaprofile(AAProfile* p, const uint8_t* order, uintptr_t order_len, const int8_t* scores, uintptr_t scores_len,
                             uintptr_t left_shift, uintptr_t right_shift) { profile_set_all(p, order, order_len, scores, scores_len, left_shift, right_shift, false); }
void block_set_all_rev_aaprofile(AAProfile* p, const uint8_t* order, uintptr_t order_len, const int8_t* scores, uintptr_t scores_len,
                                 uintptr_t left_shift, uintptr_t right_shift) { profile_set_all(p, order, order_len, scores, scores_len, left_shift, right_shift, true); }
void block_set_gap_open_C_aaprofile(AAProfile* p, uintptr_t i, int8_t gap) { if (gap >= 0) die("Gap open cost must be negative!"); p->gap_open_C.at(i) = gap; }
void block_set_gap_close_C_aaprofile(AAProfile* p, uintptr_t i, int8_t gap) { p->gap_close_C.at(i) = gap; }
void block_set_gap_open_R_aaprofile(AAProfile* p, uintptr_t i, int8_t gap) { if (gap >= 0) die("Gap open cost must be negative!"); p->gap_open_R.at(i) = gap; }
void block_set_all_gap_open_C_aaprofile(AAProfile* p, int8_t gap) { if (gap >= 0) die("Gap open cost must be negative!"); std::fill(p->gap_open_C.begin(), p->gap_open_C.begin() + p->str_len + 1, (int16_t)gap); }
void block_set_all_gap_close_C_aaprofile(AAProfile* p, int8_t gap) { std::fill(p->gap_close_C.begin(), p->gap_close_C.begin() + p->str_len + 1, (int16_t)gap); }
void block_set_all_gap_open_R_aaprofile(AAProfile* p, int8_t gap) { if (gap >= 0) die("Gap open cost must be negative!"); std::fill(p->gap_open_R.begin(), p->gap_open_R.begin() + p->str_len + 1, (int16_t)gap); }
int8_t block_get_aaprofile(const AAProfile* p, uintptr_t i, uint8_t b) {
    b = upper(b);
    if (!(b >= 'A' && b <= 'Z' + 1)) die("AAProfile::get: byte must be in 'A'..='['");
    return p->pos_aa.at(i * 32 + (b - 'A'));
}
int8_t block_get_gap_extend_aaprofile(const AAProfile* p) { return p->gap_extend; }
// Part 2: bulk form of set / set_gap_* for bindings that already hold the profile as arrays. Copies the first
// `positions` rows of pos_aa ([position][32]) and entries of the three gap arrays; no range checks beyond the length.
int ba_aaprofile_set_raw(AAProfile* p, const int8_t* pos_aa, const int8_t* gap_open_C, const int8_t* gap_close_C,
                         const int8_t* gap_open_R, uintptr_t positions) {
    if (!p || !pos_aa || !gap_open_C || !gap_close_C || !gap_open_R) return fail("null argument");
    if (positions > p->curr_len) return fail("%zu positions exceed the profile's %zu", (size_t)positions, p->curr_len);
    memcpy(p->pos_aa.data(), pos_aa, (size_t)positions * 32);
    for (size_t i = 0; i < positions; i++) { p->gap_open_C[i] = gap_open_C[i]; p->gap_close_C[i] = gap_close_C[i]; p->gap_open_R[i] = gap_open_R[i]; }
    return 0;
}
void block_free_aaprofile(AAProfile* p) { delete p; }

}  // extern "C"


// Block::align_exp / align_profile_exp over a batch (scan_block.rs:884-902, 974-992): a second (third, ...) kernel
// pass over the subset of pairs that stayed below the target score, with the min block size doubled each time.
template <class MakeBatch>
static int batch_exp(size_t n, SizeRange size, int32_t target, MakeBatch make, AlignResult* results, uintptr_t* reached_min) {
    if (!results || !reached_min) return fail("null argument");
    size_t min_size = size.min < 16 ? 16 : size.min;
    const size_t max_size = size.max < 16 ? 16 : size.max;
    std::vector<size_t> todo(n);
    for (size_t p = 0; p < n; p++) { todo[p] = p; reached_min[p] = 0; }
    while (min_size <= max_size && !todo.empty()) {
        std::unique_ptr<BaBatch> b(make(todo, SizeRange{min_size, max_size}));
        if (!b) return 1;
        if (batch_run(b.get(), nullptr)) return 1;
        const size_t m = todo.size();
        std::vector<int32_t> sc(m); std::vector<uint32_t> qi(m), ri(m), st(m);
        if (ba_batch_results(b.get(), sc.data(), qi.data(), ri.data(), nullptr, nullptr, st.data())) return 1;
        std::vector<size_t> next;
        for (size_t k = 0; k < m; k++) {
            const size_t p = todo[k];
            if (st[k]) return fail("pair %zu failed on the device (status 0x%x)", p, st[k]);
            results[p] = AlignResult{sc[k], qi[k], ri[k]};
            if (sc[k] >= target) reached_min[p] = min_size; else next.push_back(p);
        }
        todo.swap(next);
        min_size *= 2;
    }
    return 0;
}

extern "C" {
int block_batch_align_exp(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, int32_t target_score, uint32_t mode,
                          const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                          uintptr_t n, AlignResult* results, uintptr_t* reached_min) {
    if (!matrix || !pool || !q_off || !q_len || !r_off || !r_len) return fail("null argument");
    if (kind == BA_KIND_PROFILE_) return fail("use block_batch_align_profile_exp for profiles");
    mode &= ~(uint32_t)(BA_TRACE | BA_CIGAR_EQ);   // scores only: trace the finished pairs with a plain batch at reached_min
    return batch_exp(n, size, target_score, [&](const std::vector<size_t>& idx, SizeRange s) {
        return batch_build(kind, matrix, gaps, s, x_drop, mode, idx.size(), false, [&](size_t k, int w, const uint8_t** ptr, size_t* len) {
            const size_t p = idx[k];
            if (w == 0) { *ptr = pool + q_off[p]; *len = q_len[p]; } else { *ptr = pool + r_off[p]; *len = r_len[p]; }
        });
    }, results, reached_min);
}
int block_batch_align_profile_exp(const AAProfile* const* profiles, SizeRange size, int32_t x_drop, int32_t target_score, uint32_t mode,
                                  const uint8_t* pool, const uint64_t* q_off, const uint32_t* q_len, uintptr_t n,
                                  AlignResult* results, uintptr_t* reached_min) {
    if (!profiles || !pool || !q_off || !q_len || n == 0 || !profiles[0]) return fail("null argument");
    mode &= ~(uint32_t)(BA_TRACE | BA_CIGAR_EQ);
    const Gaps g{0, profiles[0]->gap_extend};
    return batch_exp(n, size, target_score, [&](const std::vector<size_t>& idx, SizeRange s) {
        return batch_build(BA_KIND_PROFILE_, nullptr, g, s, x_drop, mode, idx.size(), false,
                           [&](size_t k, int, const uint8_t** ptr, size_t* len) { *ptr = pool + q_off[idx[k]]; *len = q_len[idx[k]]; },
                           [&](size_t k) { return profiles[idx[k]]; });
    }, results, reached_min);
}
}  // extern "C"

// ------------------------------------------------------------------ batches made of ordinary batches
// A multi-device batch (one part per device) and a sized batch (one part per block range) are both a list of ordinary batches and, for
// every part, the caller's positions of its pairs. They are created and run by their own policies; the getters are written once over
// that representation (parts_*): a part whose positions are one contiguous run is written straight into the caller's buffers at its
// offset, any other part is gathered into a buffer of its own and scattered to its positions.
struct BaPartSet {
    std::vector<std::unique_ptr<BaBatch>> part;   // null: a part without pairs (a multi-device batch with more devices than pairs)
    std::vector<std::vector<uint64_t>> pos;       // part k's pairs: their positions in the caller's order, ascending
    std::vector<float> last_ms;                   // kernel time of every part in the last run
    size_t n = 0;
    uint32_t mode = 0;
    // The last run of the set was begun and did not complete for every part. The parts' own `ran` cannot say so: after a timeout in the first
    // of a sized set's chained ranges the later ones were never launched in that run and still hold the results of the run before.
    bool incomplete = false;
};
// Every getter of a set begins here: no result of any part is served unless the set's last run completed for all of them. (A set that was never
// run passes: its parts refuse what needs a run, and the exact calls need none.)
static int parts_refused(const BaPartSet* m) {
    if (!m) return fail("null batch");
    for (const auto& b : m->part)
        if (b && b->in_flight) return fail("the set has a launch in flight from a run that did not finish (run the set again: it waits for that launch first)");
    if (m->incomplete) return fail("the set's last run did not complete for every part: it has no results (run the set again)");
    return 0;
}
// Every run of a set begins here: the launches a timed-out run left in flight are waited for, under the current limit. 0: no part is in flight;
// 1: one still is (batch_wait's message stands) and nothing may be launched. A launch that ends in an error here belonged to the earlier run, which
// has failed already: the part is free again, and the run that follows starts every part afresh.
static int parts_collect(BaPartSet* m) {
    for (auto& b : m->part) {
        if (!b || !b->in_flight) continue;
        if (batch_wait(b.get(), nullptr) && b->in_flight) return 1;
    }
    return 0;
}
static bool one_run(const std::vector<uint64_t>& pos) { return !pos.empty() && pos.back() - pos.front() + 1 == pos.size(); }
// One caller array as a part sees it: the part's slice of it when the part's positions are one run, else a buffer scatter() spreads.
template <class T> struct PartOut {
    T* out;
    const std::vector<uint64_t>& pos;
    std::vector<T> tmp;
    PartOut(T* out_, const std::vector<uint64_t>& pos_) : out(out_), pos(pos_) { if (out && !one_run(pos)) tmp.resize(pos.size()); }
    T* get() { return !out ? nullptr : (tmp.empty() ? out + pos[0] : tmp.data()); }
    void scatter() const { for (size_t i = 0; i < tmp.size(); i++) out[pos[i]] = tmp[i]; }
};
static int parts_results(BaPartSet* m, int32_t* score, uint32_t* qi, uint32_t* ri, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    if (parts_refused(m)) return 1;
    for (size_t k = 0; k < m->part.size(); k++) {
        if (!m->part[k]) continue;
        const auto& pos = m->pos[k];
        PartOut<int32_t> s(score, pos);
        PartOut<uint32_t> a(qi, pos), b(ri, pos), l(cigar_len, pos), st(status, pos);
        PartOut<uint64_t> c(cells, pos);
        if (ba_batch_results(m->part[k].get(), s.get(), a.get(), b.get(), c.get(), l.get(), st.get())) return 1;
        s.scatter(); a.scatter(); b.scatter(); c.scatter(); l.scatter(); st.scatter();
    }
    return 0;
}
static int parts_cigars(BaPartSet* m, uint32_t* runs, uint64_t capacity) {   // concatenated in the caller's pair order, as ba_batch_cigars
    if (parts_refused(m)) return 1;
    std::vector<uint32_t> len(m->n, 0);
    if (parts_results(m, nullptr, nullptr, nullptr, nullptr, len.data(), nullptr)) return 1;
    std::vector<uint64_t> off(m->n + 1, 0);
    for (size_t p = 0; p < m->n; p++) off[p + 1] = off[p] + len[p];
    if (off[m->n] > capacity) return fail("cigar buffer too small: need %llu entries", (unsigned long long)off[m->n]);
    std::vector<uint32_t> tmp;
    for (size_t k = 0; k < m->part.size(); k++) {
        const auto& pos = m->pos[k];
        uint64_t total = 0;
        for (uint64_t p : pos) total += len[p];
        if (!total) continue;
        if (one_run(pos)) {
            if (ba_batch_cigars(m->part[k].get(), runs + off[pos[0]], total)) return 1;
            continue;
        }
        tmp.resize(total);
        if (ba_batch_cigars(m->part[k].get(), tmp.data(), total)) return 1;
        uint64_t at = 0;
        for (uint64_t p : pos) { if (len[p]) std::memcpy(runs + off[p], tmp.data() + at, (size_t)len[p] * 4); at += len[p]; }
    }
    return 0;
}
static int parts_stats(BaPartSet* m, BaAlignStats* out) {
    if (parts_refused(m)) return 1;
    if (!out) return fail("null argument");
    for (size_t k = 0; k < m->part.size(); k++) {
        if (!m->part[k]) continue;
        PartOut<BaAlignStats> o(out, m->pos[k]);
        if (ba_batch_stats(m->part[k].get(), o.get())) return 1;
        o.scatter();
    }
    return 0;
}
static int parts_exact(BaPartSet* m, uint32_t what, int32_t x_drop, const uint32_t* which, size_t n_which, BaExact* out) {   // every part computes its own pairs
    if (parts_refused(m)) return 1;
    if (!out) return fail("null argument: out");
    const size_t cnt = which ? n_which : m->n;
    std::vector<uint32_t> part_of(m->n), local_of(m->n);
    for (size_t k = 0; k < m->part.size(); k++)
        for (size_t i = 0; i < m->pos[k].size(); i++) { part_of[m->pos[k][i]] = (uint32_t)k; local_of[m->pos[k][i]] = (uint32_t)i; }
    std::vector<std::vector<uint32_t>> local(m->part.size()), at(m->part.size());   // per part: its pairs of the request, and their records
    for (size_t k = 0; k < cnt; k++) {
        const uint32_t p = which ? which[k] : (uint32_t)k;
        if (p >= m->n) return fail("exact: which[%zu] = %u is out of range (the batch holds %zu pairs)", k, p, m->n);
        local[part_of[p]].push_back(local_of[p]); at[part_of[p]].push_back((uint32_t)k);
    }
    std::vector<BaExact> tmp;
    for (size_t k = 0; k < m->part.size(); k++) {
        if (local[k].empty()) continue;
        tmp.resize(local[k].size());
        if (batch_exact(m->part[k].get(), what, x_drop, local[k].data(), local[k].size(), tmp.data())) return 1;
        for (size_t i = 0; i < tmp.size(); i++) out[at[k][i]] = tmp[i];
    }
    return 0;
}
// ... and its own paths: the parts' offsets become run counts in the caller's order, then offsets; with `runs`, every part's runs are
// scattered to them (a part answers that second call from its device buffers)
template <class Rec>
static int parts_exact_cigars(BaPartSet* m, uint32_t what, int32_t x_drop, const uint32_t* which, size_t n_which, Rec* out, uint64_t* run_off,
                              uint32_t* runs, uint64_t capacity) {
    if (parts_refused(m)) return 1;
    if (!out) return fail("null argument: out");
    if (!run_off) return fail("null argument: run_off");
    const size_t cnt = which ? n_which : m->n;
    std::vector<uint32_t> part_of(m->n), local_of(m->n);
    for (size_t k = 0; k < m->part.size(); k++)
        for (size_t i = 0; i < m->pos[k].size(); i++) { part_of[m->pos[k][i]] = (uint32_t)k; local_of[m->pos[k][i]] = (uint32_t)i; }
    std::vector<std::vector<uint32_t>> local(m->part.size()), at(m->part.size());
    for (size_t k = 0; k < cnt; k++) {
        const uint32_t p = which ? which[k] : (uint32_t)k;
        if (p >= m->n) return fail("exact: which[%zu] = %u is out of range (the batch holds %zu pairs)", k, p, m->n);
        local[part_of[p]].push_back(local_of[p]); at[part_of[p]].push_back((uint32_t)k);
    }
    std::vector<Rec> tmp;
    std::vector<std::vector<uint64_t>> po(m->part.size());
    std::fill(run_off, run_off + cnt + 1, 0);
    for (size_t k = 0; k < m->part.size(); k++) {
        if (local[k].empty()) continue;
        tmp.resize(local[k].size()); po[k].resize(local[k].size() + 1);
        if (batch_exact_cigars(m->part[k].get(), what, x_drop, local[k].data(), local[k].size(), tmp.data(), po[k].data(), nullptr, 0)) return 1;
        for (size_t i = 0; i < tmp.size(); i++) { out[at[k][i]] = tmp[i]; run_off[at[k][i] + 1] = po[k][i + 1] - po[k][i]; }
    }
    for (size_t k = 0; k < cnt; k++) run_off[k + 1] += run_off[k];
    if (!runs) return 0;
    if (capacity < run_off[cnt]) return fail("exact: the runs buffer holds %llu runs, the request has %llu", (unsigned long long)capacity, (unsigned long long)run_off[cnt]);
    std::vector<uint32_t> pr;
    for (size_t k = 0; k < m->part.size(); k++) {
        if (local[k].empty()) continue;
        tmp.resize(local[k].size()); pr.resize((size_t)std::max<uint64_t>(po[k].back(), 1));
        if (batch_exact_cigars(m->part[k].get(), what, x_drop, local[k].data(), local[k].size(), tmp.data(), po[k].data(), pr.data(), po[k].back())) return 1;
        for (size_t i = 0; i < tmp.size(); i++) std::copy(pr.begin() + po[k][i], pr.begin() + po[k][i + 1], runs + run_off[at[k][i]]);
    }
    return 0;
}
static int parts_text(BaPartSet* m, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) {   // sized per part, then rendered per part
    if (parts_refused(m)) return 1;
    if (!offsets) return fail("null argument: offsets");
    if (text_check(BA_KIND_NUC, m->mode, what)) return 1;   // (the kind's refusals come from the parts)
    std::vector<std::vector<uint64_t>> po(m->part.size());   // every part's own offsets
    std::fill(offsets, offsets + m->n + 1, 0);
    for (size_t k = 0; k < m->part.size(); k++) {
        if (!m->part[k]) continue;
        const auto& pos = m->pos[k];
        po[k].resize(pos.size() + 1);
        if (batch_text_device(m->part[k].get(), what, po[k].data(), nullptr, 0)) return 1;
        for (size_t i = 0; i < pos.size(); i++) offsets[pos[i] + 1] = po[k][i + 1] - po[k][i];
    }
    for (size_t p = 0; p < m->n; p++) offsets[p + 1] += offsets[p];
    if (!text) return 0;
    if (capacity < offsets[m->n])
        return fail("text buffer too small: the text needs %llu bytes, the buffer holds %llu", (unsigned long long)offsets[m->n], (unsigned long long)capacity);
    std::vector<char> tmp;
    for (size_t k = 0; k < m->part.size(); k++) {
        const auto& pos = m->pos[k];
        const uint64_t total = m->part[k] ? po[k].back() : 0;
        if (!total) continue;
        if (one_run(pos)) {
            if (batch_text_device(m->part[k].get(), what, po[k].data(), text + offsets[pos[0]], total)) return 1;
            continue;
        }
        tmp.resize(total);
        if (batch_text_device(m->part[k].get(), what, po[k].data(), tmp.data(), total)) return 1;
        for (size_t i = 0; i < pos.size(); i++)
            if (po[k][i + 1] > po[k][i]) std::memcpy(text + offsets[pos[i]], tmp.data() + po[k][i], po[k][i + 1] - po[k][i]);
    }
    return 0;
}

// ---- one batch over several GPUs
// Pairs are independent, so a batch shards without any exchange step: contiguous slices of the caller's pair
// list, balanced by cost (|q| + |r|, what the number of driver steps follows), one BaBatch per device, each created by its
// own host thread (packing and upload run in parallel), launched on its own stream; results come back in the caller's order.
extern "C" int ba_shard_slices(const uint32_t* q_len, const uint32_t* r_len, uintptr_t n, int parts, uint64_t* bounds) {
    if (!q_len || !r_len || !bounds || parts < 1) return fail("null argument");
    std::vector<uint64_t> pre(n + 1, 0);
    for (size_t p = 0; p < n; p++) pre[p + 1] = pre[p] + (uint64_t)q_len[p] + r_len[p] + 16;   // (+16: even empty pairs cost a launch slot)
    bounds[0] = 0;
    for (int k = 1; k < parts; k++) {
        const uint64_t target = pre[n] / (uint64_t)parts * (uint64_t)k + pre[n] % (uint64_t)parts * (uint64_t)k / (uint64_t)parts;
        size_t lo = std::lower_bound(pre.begin(), pre.end(), target) - pre.begin();
        if (lo > n) lo = n;
        if (lo < bounds[k - 1]) lo = bounds[k - 1];
        bounds[k] = lo;
    }
    bounds[parts] = n;
    return 0;
}

struct BaMultiBatch : BaPartSet {
    std::vector<uint64_t> bounds;     // part k holds the caller's pairs [bounds[k], bounds[k + 1])
};

extern "C" {
BaMultiBatch* ba_multibatch_create(int kind, const void* matrix, Gaps gaps, SizeRange size, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                   const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n,
                                   const int* devices, int n_devices) {
    if (!matrix || !pool || !q_off || !q_len || !r_off || !r_len || !devices || n_devices < 1) { fail("null argument"); return nullptr; }
    if (n == 0) { fail("batch must hold at least one pair"); return nullptr; }
    const int have = ba_device_count();
    for (int k = 0; k < n_devices; k++)
        if (devices[k] < 0 || devices[k] >= have) { fail("device %d out of range (%d devices)", devices[k], have); return nullptr; }
    std::unique_ptr<BaMultiBatch> m(new BaMultiBatch);
    m->n = n; m->mode = mode;
    m->bounds.resize(n_devices + 1);
    if (ba_shard_slices(q_len, r_len, n, n_devices, m->bounds.data())) return nullptr;
    m->part.resize(n_devices);
    m->pos.resize(n_devices);
    std::vector<std::string> errs(n_devices);
    auto build = [&](int k) {
        const size_t lo = m->bounds[k], cnt = m->bounds[k + 1] - lo;
        if (cnt == 0) return;                                  // more devices than pairs: this one stays idle
        for (size_t p = lo; p < lo + cnt; p++) m->pos[k].push_back(p);
        g_device = devices[k];                                 // (thread-local)
        BaBatch* b = ba_batch_create(kind, matrix, gaps, size, x_drop, mode, pool, q_off + lo, q_len + lo, r_off + lo, r_len + lo, cnt);
        if (!b) errs[k] = g_err; else m->part[k].reset(b);
    };
    std::vector<std::thread> th;
    for (int k = 1; k < n_devices; k++) th.emplace_back(build, k);
    const int keep = g_device;
    build(0);
    g_device = keep;
    for (auto& t : th) t.join();
    for (int k = 0; k < n_devices; k++)
        if (!errs[k].empty()) { fail("device %d: %s", devices[k], errs[k].c_str()); return nullptr; }
    return m.release();
}
int ba_multibatch_run(BaMultiBatch* m, float* kernel_ms) {
    if (!m) return fail("null batch");
    // all devices first, then collect. A failure does not leave the other parts in flight: every part that was launched is
    // waited for before the first error is reported -- except after a timeout: that part stays in flight, the set has no results
    // (incomplete), and the next run collects it before it launches anything.
    if (parts_collect(m)) return 1;
    m->incomplete = true;
    std::string first_err;
    for (auto& b : m->part) {
        if (!b || !first_err.empty()) continue;
        if (batch_launch(b.get())) first_err = g_err;
    }
    float worst = 0;
    m->last_ms.assign(m->part.size(), 0.f);
    for (size_t k = 0; k < m->part.size(); k++) {
        auto& b = m->part[k];
        if (!b || !b->in_flight) continue;
        float ms = 0;
        if (batch_wait(b.get(), &ms)) { if (first_err.empty()) first_err = g_err; continue; }   // (batch_wait itself says whether the part is still in flight: a timeout leaves it so)
        m->last_ms[k] = ms;
        worst = std::max(worst, ms);
    }
    if (!first_err.empty()) return fail("%s", first_err.c_str());
    m->incomplete = false;
    if (kernel_ms) *kernel_ms = worst;
    return 0;
}
int ba_multibatch_results(BaMultiBatch* m, int32_t* score, uint32_t* qi, uint32_t* ri, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    return parts_results(m, score, qi, ri, cells, cigar_len, status);
}
int ba_multibatch_cigars(BaMultiBatch* m, uint32_t* runs, uint64_t capacity) { return parts_cigars(m, runs, capacity); }
int ba_multibatch_stats(BaMultiBatch* m, BaAlignStats* out) { return parts_stats(m, out); }
int ba_multibatch_exact_cigars(BaMultiBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out, uint64_t* run_off,
                               uint32_t* runs, uint64_t capacity) {
    return parts_exact_cigars(m, what, x_drop, which, n_which, out, run_off, runs, capacity);
}
int ba_multibatch_exact_paths(BaMultiBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExactPath* out, uint64_t* run_off,
                              uint32_t* runs, uintptr_t runs_cap) {
    if (exact_paths_args(out, run_off)) return 1;
    return parts_exact_cigars(m, what, x_drop, which, n_which, out, run_off, runs, runs_cap);
}
int ba_multibatch_exact(BaMultiBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out) { return parts_exact(m, what, x_drop, which, n_which, out); }
int ba_multibatch_text(BaMultiBatch* m, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) { return parts_text(m, what, offsets, text, capacity); }
int ba_multibatch_kernel_ms(BaMultiBatch* m, float* ms, int capacity) {   // per slice, of the last run; returns the number of slices
    if (!m) return -1;
    if (parts_refused(m)) return -1;   // (the times of a run that did not complete are no times: ba_last_error says why)
    for (int k = 0; k < capacity && k < (int)m->last_ms.size(); k++) ms[k] = m->last_ms[k];
    return (int)m->part.size();
}
int ba_multibatch_parts(BaMultiBatch* m, uint64_t* bounds, int capacity) {   // slice boundaries (n_devices + 1 entries); returns n_devices
    if (!m) return -1;
    for (int k = 0; k < capacity && k < (int)m->bounds.size(); k++) bounds[k] = m->bounds[k];
    return (int)m->part.size();
}
void ba_multibatch_destroy(BaMultiBatch* m) { delete m; }

// ---- every pair with its own block range (lib.rs:109-111 percent_len per pair, as examples/nanopore_bench_global.rs:163,171 calls it):
// pairs are binned by (min, max), every bin is an ordinary batch of this library -- the multi-pair kernels where the bin's minimum size has one --
// launched together on the device (ba_sized_batch_run); results and CIGAR runs come back in the caller's order.
struct BaSizedBatch : BaPartSet {
    std::vector<SizeRange> range;                 // part k's block range
    std::vector<double> work;                     // part k's share of the work (residues x maximum block size): launch order, memory share
};
BaSizedBatch* ba_sized_batch_create(int kind, const void* matrix, Gaps gaps, const SizeRange* size_per_pair, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                    const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n) {
    if (!matrix || !size_per_pair || !pool || !q_off || !q_len || !r_off || !r_len) { fail("null argument"); return nullptr; }
    if (n == 0) { fail("batch must hold at least one pair"); return nullptr; }
    if (n >= (1ull << 32)) { fail("too many pairs"); return nullptr; }
    std::unique_ptr<BaSizedBatch> m(new BaSizedBatch);
    m->n = n; m->mode = mode;
    std::map<std::pair<uintptr_t, uintptr_t>, size_t> cls;
    for (size_t p = 0; p < n; p++) {
        const auto key = std::make_pair(size_per_pair[p].min, size_per_pair[p].max);
        auto it = cls.find(key);
        if (it == cls.end()) { it = cls.emplace(key, m->pos.size()).first; m->pos.emplace_back(); m->range.push_back(size_per_pair[p]); }
        m->pos[it->second].push_back(p);
    }
    m->part.resize(m->pos.size());
    // every range's batch gets a share of the free device memory in proportion to what its trace stacks ask for (residues x maximum block size)
    std::vector<double> weight(m->pos.size(), 0.0);
    double weight_left = 0;
    for (size_t k = 0; k < m->pos.size(); k++) {
        for (uint64_t p : m->pos[k]) weight[k] += ((double)q_len[p] + r_len[p] + 64.0) * (double)m->range[k].max;
        weight_left += weight[k];
    }
    m->work = weight;
    struct CapReset { ~CapReset() { g_mem_cap = ~0ull; } } cap_reset;
    for (size_t k = 0; k < m->pos.size(); k++) {
        {
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            g_mem_cap = m->pos.size() > 1 ? (uint64_t)((double)free_b * 0.95 * (weight[k] / std::max(weight_left, 1.0))) : ~0ull;
            g_mem_cap = std::max<uint64_t>(g_mem_cap, 3ull << 30);   // (batch_plan keeps 1 GB aside; a range of a few pairs still needs its scratch)
            weight_left -= weight[k];
        }
        const auto& ix = m->pos[k];
        std::vector<uint64_t> qo(ix.size()), ro(ix.size());
        std::vector<uint32_t> ql(ix.size()), rl(ix.size());
        for (size_t i = 0; i < ix.size(); i++) { qo[i] = q_off[ix[i]]; ro[i] = r_off[ix[i]]; ql[i] = q_len[ix[i]]; rl[i] = r_len[ix[i]]; }
        BaBatch* b = ba_batch_create(kind, matrix, gaps, m->range[k], x_drop, mode, pool, qo.data(), ql.data(), ro.data(), rl.data(), ix.size());
        if (!b) { const std::string e = g_err; fail("block range %llu..%llu (%llu pairs): %s", (unsigned long long)m->range[k].min, (unsigned long long)m->range[k].max, (unsigned long long)ix.size(), e.c_str()); return nullptr; }
        m->part[k].reset(b);
    }
    return m.release();
}
BaSizedBatch* ba_sized_batch_create_percent(int kind, const void* matrix, Gaps gaps, float min_percent, float max_percent, int32_t x_drop, uint32_t mode, const uint8_t* pool,
                                            const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len, uintptr_t n) {
    if (!q_len || !r_len) { fail("null argument"); return nullptr; }
    std::vector<SizeRange> sz(n);
    for (size_t p = 0; p < n; p++) {   // examples/nanopore_bench_global.rs:144-171: both percentages of the longer sequence's length
        const uintptr_t len = std::max(q_len[p], r_len[p]);
        sz[p].min = block_percent_len(len, min_percent); sz[p].max = block_percent_len(len, max_percent);
    }
    return ba_sized_batch_create(kind, matrix, gaps, sz.data(), x_drop, mode, pool, q_off, q_len, r_off, r_len, n);
}
int ba_sized_batch_run(BaSizedBatch* m, float* kernel_ms) {
    if (!m) return fail("null batch");
    if (parts_collect(m)) return 1;   // (what a timed-out run left in flight; still running: nothing is launched)
    m->incomplete = true;
    // Round 5: all ranges' launches at once, each on its batch's own stream, the ones with the most work first: a range of a few thousand pairs
    // does not fill the device (its grid is what its pairs need), and the long ranges' launches end with a few long pairs. kernel_ms: the host's
    // clock from the first launch to the last completion (the device is idle before: the previous run was waited for).
    m->last_ms.assign(m->part.size(), 0.f);
    std::vector<size_t> order(m->part.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return m->work[a] > m->work[b]; });
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    std::string first_err;
    // Round 6: a launch whose waves wait for each other -- the hand-off ring of a traced batch (its traceback waves and helpers wait for the fill waves'
    // hand-offs), k_multi's end-of-batch slot donation (its idle waves wait until every fill wave has been counted) -- needs all of its workgroups resident
    // to be sure to end. Alone it is (the grid is what the device holds); beside launches that simply run out it still is, later; but two or more such
    // launches that each hold a part of the device wait for workgroups the other's waiting waves keep out (three ranges of k_multi in one per-pair-ranges
    // batch: 9 .. 25 s instead of 0.2, every wait ended by a time-out). So: the ranges without such waits all at once, the ones with them one after the
    // other beside those.
    auto waits_inside = [&](const BaBatch* b) { return b->tb_stride != 0 || (b->multi && (b->mode & BA_TRACE) && b->donate.p != nullptr); };
    std::vector<size_t> free_run, chained;
    for (size_t k : order) (waits_inside(m->part[k].get()) ? chained : free_run).push_back(k);
    std::vector<char> launched(m->part.size(), 0);
    // launched[k]: 1 = to be waited for in this call; 2 = its wait timed out, the part is still in flight: not waited for a second time here, and
    // not forgotten -- the set stays incomplete, and the next run collects it (parts_collect)
    auto wait_one = [&](size_t k) {
        float ms = 0;
        if (ba_batch_wait(m->part[k].get(), &ms) && !rc) { rc = 1; first_err = g_err; }
        m->last_ms[k] = ms; launched[k] = m->part[k]->in_flight ? 2 : 0;
    };
    auto launch_one = [&](size_t k) { if (rc) return; if (ba_batch_launch(m->part[k].get())) { rc = 1; first_err = g_err; } else launched[k] = 1; };
    if (!chained.empty()) launch_one(chained[0]);   // (the longest chain first: the other ranges fill the device around it)
    for (size_t k : free_run) launch_one(k);
    for (size_t i = 0; i < chained.size(); i++) {
        if (launched[chained[i]] == 1) wait_one(chained[i]);
        if (i + 1 < chained.size()) launch_one(chained[i + 1]);
    }
    for (size_t k : free_run) if (launched[k] == 1) wait_one(k);   // (also after a failed launch: nothing but a timed-out part is left in flight)
    for (size_t k = 0; k < launched.size(); k++) if (launched[k] == 1) wait_one(k);
    if (rc) return fail("%s", first_err.c_str());
    m->incomplete = false;
    if (kernel_ms) *kernel_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
int ba_sized_batch_results(BaSizedBatch* m, int32_t* score, uint32_t* qi, uint32_t* ri, uint64_t* cells, uint32_t* cigar_len, uint32_t* status) {
    return parts_results(m, score, qi, ri, cells, cigar_len, status);
}
int ba_sized_batch_cigars(BaSizedBatch* m, uint32_t* runs, uint64_t capacity) { return parts_cigars(m, runs, capacity); }
int ba_sized_batch_stats(BaSizedBatch* m, BaAlignStats* out) { return parts_stats(m, out); }
int ba_sized_batch_exact_cigars(BaSizedBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out, uint64_t* run_off,
                                uint32_t* runs, uint64_t capacity) {
    return parts_exact_cigars(m, what, x_drop, which, n_which, out, run_off, runs, capacity);
}
int ba_sized_batch_exact_paths(BaSizedBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExactPath* out, uint64_t* run_off,
                               uint32_t* runs, uintptr_t runs_cap) {
    if (exact_paths_args(out, run_off)) return 1;
    return parts_exact_cigars(m, what, x_drop, which, n_which, out, run_off, runs, runs_cap);
}
int ba_sized_batch_exact(BaSizedBatch* m, uint32_t what, int32_t x_drop, const uint32_t* which, uintptr_t n_which, BaExact* out) { return parts_exact(m, what, x_drop, which, n_which, out); }
int ba_sized_batch_text(BaSizedBatch* m, uint32_t what, uint64_t* offsets, char* text, uint64_t capacity) { return parts_text(m, what, offsets, text, capacity); }
int ba_sized_batch_classes(BaSizedBatch* m, SizeRange* ranges, uint64_t* counts, int32_t* kernels, float* kernel_ms, int capacity) {   // the bins; returns their number
    if (!m) return -1;
    if (parts_refused(m)) return -1;   // (as ba_multibatch_kernel_ms)
    for (int k = 0; k < capacity && k < (int)m->part.size(); k++) {
        if (ranges) ranges[k] = m->range[k];
        if (counts) counts[k] = m->pos[k].size();
        if (kernels) kernels[k] = ba_batch_kernel(m->part[k].get());
        if (kernel_ms) kernel_ms[k] = k < (int)m->last_ms.size() ? m->last_ms[k] : 0.f;
    }
    return (int)m->part.size();
}
void ba_sized_batch_destroy(BaSizedBatch* m) { delete m; }
}  // extern "C"

// ------------------------------------------------------------------ Block handles (Part 1 + generic)
// Like the reference's Block (scan_block.rs:798-805, 1280-1340: Block::new allocates, align never does), a handle owns its
// device state from creation: stream, events, the two image slots, one trace slot, the rectangle list, the CIGAR buffer
// and the checkpoint scratch, sized for any pair with |q| + |r| <= query_len + reference_len and any block size up to
// max_size. An align uploads one buffer (images + the per-pair words), launches one workgroup and reads one 64-byte
// record back; nothing is allocated or freed.
struct HandleUpload {   // head of BaBatch::hblk; the images follow at `images`
    uint64_t q_off, r_off, cig_off[2];
    uint32_t q_len, r_len, work_counter, pad_;
    static constexpr size_t images = 64;
};
struct HandleResult {   // BaBatch::rblk
    int32_t score; uint32_t query_idx, reference_idx, cig_len, status, nblocks, slot, trace_words;
    unsigned long long cells; uint32_t pad_[6];
};
static_assert(sizeof(HandleUpload) <= HandleUpload::images && sizeof(HandleResult) == 64, "handle records");

struct BlockImpl {
    uint32_t mode;                 // BA_TRACE | BA_X_DROP | ...
    size_t query_len, reference_len, max_size;   // upper bounds from Block::new (scan_block.rs:798-805)
    AlignResult res{0, 0, 0};
    std::unique_ptr<BaBatch> dev;                // persistent device state (created with the handle when a device is usable)
    std::vector<uint8_t> staging;                // host image of hblk
    int8_t matrix_image[1024] = {0};             // host image of the matrix last uploaded
    bool matrix_valid = false;
    uint32_t last_ql = 0, last_rl = 0, last_nblocks = 0, last_slot = 0;
    bool aligned = false;
};

static uint64_t handle_trace_stride(size_t max_size, uint64_t maxlen2, uint32_t mode) {   // Trace::new's bound, scan_block.rs:1363-1366 (+ zero mask, + slack)
    return (uint64_t)(max_size / 16) * (maxlen2 + 2 * max_size) * 2 * ((mode & BA_LOCAL_START) ? 2 : 1) + 64;
}

// Allocate a handle's device state. Returns 0, or non-zero with the message in g_err (the caller decides whether that is fatal).
static int handle_prepare(BlockImpl* h) {
    if (ensure_device()) return 1;
    std::unique_ptr<BaBatch> b(new BaBatch);
    b->device = g_device; b->handle_mode = true; b->n = 1;
    const size_t max_size = h->max_size < 16 ? 16 : h->max_size, sum = h->query_len + h->reference_len;
    if (sum > 0x3fffffffu) return fail("sequences too long");
    const bool trace = h->mode & BA_TRACE;
    const size_t pad = max_size + 16;
    // either sequence may be as long as the sum; the reference side may be an AAProfile image instead
    const uint64_t seq_img = (1 + sum + pad + 3 + 8) & ~(size_t)7;
    const uint64_t ref_img = std::max<uint64_t>(seq_img, (ba::profile_image_bytes((uint32_t)sum, (uint32_t)max_size) + 7) & ~7ull);
    b->cap_pool = HandleUpload::images + seq_img + ref_img + POOL_SLACK;
    b->cap_maxlen2 = sum + 2; b->cap_n = 1; b->cap_cig = sum + 1;
    b->trace_stride = trace ? handle_trace_stride(max_size, b->cap_maxlen2, h->mode) : 0;
    b->blocks_stride = trace ? b->cap_maxlen2 : 0;
    if (b->trace_stride >= (1ull << 30)) return fail("trace stack of %llu words exceeds the 2^30 limit", (unsigned long long)b->trace_stride);
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) return fail("hipEventCreate failed");
    if (b->hblk.alloc(b->cap_pool) || b->rblk.alloc(sizeof(HandleResult)) || b->matrix.alloc(1024) || b->cig_ops.alloc((trace ? b->cap_cig : 1) * 4) ||
        b->trace.alloc(b->trace_stride * 4) || b->blocks.alloc(b->blocks_stride * sizeof(BlockRec)) ||
        b->ckpt.alloc((size_t)ba::WAVES_PER_WG * 8 * max_size * sizeof(short)) ||
        b->big.alloc(max_size > 2048 ? (size_t)ba::WAVES_PER_WG * ba::big_wave_shorts((uint32_t)max_size) * sizeof(short) : 0) || b->prof.alloc(2048) || b->tb_ctrl.alloc(256) ||
        b->tb_queue.alloc(4) || b->slot_free.alloc(4) || b->slot_info.alloc(sizeof(ba::SlotInfo))) return 1;
    uint8_t* hb = b->hblk.as<uint8_t>(); uint8_t* rb = b->rblk.as<uint8_t>();
    b->pool.view(hb, b->cap_pool);   // the images' offsets are relative to the start of hblk
    b->q_off.view(hb + offsetof(HandleUpload, q_off), 8); b->r_off.view(hb + offsetof(HandleUpload, r_off), 8);
    b->cig_off.view(hb + offsetof(HandleUpload, cig_off), 16);
    b->q_len.view(hb + offsetof(HandleUpload, q_len), 4); b->r_len.view(hb + offsetof(HandleUpload, r_len), 4);
    b->counter.view(hb + offsetof(HandleUpload, work_counter), 4);
    b->score.view(rb + offsetof(HandleResult, score), 4); b->qidx.view(rb + offsetof(HandleResult, query_idx), 4);
    b->ridx.view(rb + offsetof(HandleResult, reference_idx), 4); b->cig_len.view(rb + offsetof(HandleResult, cig_len), 4);
    b->status.view(rb + offsetof(HandleResult, status), 4); b->nblocks.view(rb + offsetof(HandleResult, nblocks), 4);
    b->pair_slot.view(rb + offsetof(HandleResult, slot), 4); b->trace_words.view(rb + offsetof(HandleResult, trace_words), 4);
    b->cells.view(rb + offsetof(HandleResult, cells), 8);
    b->grid = 1; b->slots = 1; b->slots_per_wave = 0; b->tb_stride = 0;   // (slots_per_wave 0: whichever wave takes the pair uses slot 0)
    b->n_fill_waves = ba::WAVES_PER_WG; b->tb_qsize = 1;
    h->staging.assign(b->cap_pool, 0);
    h->dev = std::move(b);
    return 0;
}

// One alignment through a handle's persistent state. `profile` non-null: sequence-to-profile (kind PROFILE).
// q_s / r_s: a padded image's bytes as the reference keeps them (scan_block.rs:1790-1812: index 0 is the NULL pad, then the converted
// sequence); r_s unused with a profile.
static void handle_align(BlockImpl* h, int kind, const uint8_t* q_s, size_t q_len, const uint8_t* r_s, size_t r_len, const AAProfile* profile, const void* matrix,
                         Gaps g, size_t min_size, size_t max_size, int32_t x) {
    if (!h->dev && handle_prepare(h)) die("%s", g_err.c_str());
    BaBatch* b = h->dev.get();
    if (hipSetDevice(b->device) != hipSuccess) die("hipSetDevice failed");
    const int pc = pclass_of(max_size);
    if (pc < 0) die("max block size %zu not supported by the HIP backend (16..%zu)", max_size, (size_t)BA_MAX_BLOCK);
    const uint32_t mode = h->mode & ~(uint32_t)BA_CIGAR_EQ;
    const bool trace = mode & BA_TRACE;
    if ((mode & BA_FREE_QUERY_END_GAPS) && !(min_size > q_len)) die("Min block size must be larger than the query length for FREE_QUERY_END_GAPS!");   // scan_block.rs:860-862
    b->kind = kind; b->mode = mode; b->min_size = (uint32_t)min_size; b->max_size = (uint32_t)max_size; b->pclass = (uint32_t)pc;
    b->gap_open = g.open; b->gap_extend = g.extend; b->x_drop = x;
    b->lds = ba::lds_wg_bytes_h(kind, lds_class_cells(pc)) + (trace ? ba::TB_LDS_BYTES : 0u);
    // ---- the upload: per-pair words + the two padded images (scan_block.rs:1798-1812), built in the handle's staging buffer
    const size_t pad = max_size + 16;
    const uint32_t ql = (uint32_t)q_len, rl = (uint32_t)(profile ? profile->str_len : r_len);
    HandleUpload hu{};
    hu.q_off = HandleUpload::images; hu.q_len = ql; hu.r_len = rl; hu.work_counter = 0;
    const size_t q_img = (1 + (size_t)ql + pad + 3 + 8) & ~(size_t)7;
    hu.r_off = hu.q_off + q_img;
    const size_t r_img = profile ? (size_t)ba::profile_image_bytes(rl, (uint32_t)max_size) : ((1 + (size_t)rl + pad + 3) & ~(size_t)3);
    const size_t used = (size_t)hu.r_off + r_img + POOL_SLACK;
    if (used > b->cap_pool) die("sequence lengths exceed the bounds this Block was created with");
    hu.cig_off[0] = 0; hu.cig_off[1] = (uint64_t)ql + rl + 1;
    uint8_t* st = h->staging.data();
    memcpy(st, &hu, sizeof hu);
    const uint8_t nb = null_byte(kind);
    uint8_t* qi = st + hu.q_off;
    qi[0] = nb; memcpy(qi + 1, q_s + 1, ql); memset(qi + 1 + ql, nb, q_img - 1 - ql);
    uint8_t* ri = st + hu.r_off;
    if (profile) profile_image(profile, ba::profile_positions(rl, (uint32_t)max_size), ri);
    else { ri[0] = nb; memcpy(ri + 1, r_s + 1, rl); memset(ri + 1 + rl, nb, r_img - 1 - rl); }
    memset(st + hu.r_off + r_img, nb, POOL_SLACK);
    b->pool_bytes = used; b->cig_total = trace ? hu.cig_off[1] : 0;
    b->h_q_off.assign(1, hu.q_off); b->h_r_off.assign(1, hu.r_off);
    hipError_t e = hipMemcpyAsync(b->hblk.p, st, used, hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess && b->matrix.p) {
        const size_t mat_bytes = kind == BA_KIND_AA ? 27 * 32 : (kind == BA_KIND_NUC ? 8 * 16 : (kind == BA_KIND_BYTES ? 2 : 0));
        // (the image lives in the handle: the source of an asynchronous copy has to outlive the stream synchronisation;
        // unchanged matrices are not uploaded again)
        int8_t tmp[1024] = {0};
        if (kind == BA_KIND_BYTES) { const ByteMatrix* bm = (const ByteMatrix*)matrix; tmp[0] = bm->match_score; tmp[1] = bm->mismatch_score; }
        else if (mat_bytes) memcpy(tmp, matrix, mat_bytes);
        if (mat_bytes && (!h->matrix_valid || memcmp(tmp, h->matrix_image, 1024) != 0)) {
            memcpy(h->matrix_image, tmp, 1024);
            e = hipMemcpyAsync(b->matrix.p, h->matrix_image, 1024, hipMemcpyHostToDevice, b->stream);
            h->matrix_valid = e == hipSuccess;
        }
    }
    if (e != hipSuccess) die("hipMemcpy H2D failed: %s", hipGetErrorString(e));
    b->in_flight = false; b->ran = false;
    if (batch_run(b, nullptr)) die("%s", g_err.c_str());
    HandleResult hr;
    if (hipMemcpy(&hr, b->rblk.p, sizeof hr, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy D2H failed");
    if (hr.status) die("device alignment failed (status 0x%x)", hr.status);
    h->res = AlignResult{hr.score, hr.query_idx, hr.reference_idx};
    h->last_ql = ql; h->last_rl = rl; h->last_nblocks = hr.nblocks; h->last_slot = hr.slot; h->aligned = true;
}

static BlockImpl* block_new_impl(uint32_t mode, size_t query_len, size_t reference_len, size_t max_size) {
    if (max_size == 0 || (max_size & (max_size - 1))) die("Block size must be a power of two!");
    BlockImpl* b = new BlockImpl;
    b->mode = mode; b->query_len = query_len; b->reference_len = reference_len; b->max_size = max_size;
    // Block::new allocates (scan_block.rs:798-805). Without a usable device the handle still exists -- precondition checks
    // work anywhere -- and the first align reports the missing device.
    if (pclass_of(max_size < 16 ? 16 : max_size) >= 0) (void)handle_prepare(b);
    return b;
}

static void block_align_impl(BlockImpl* b, int kind, const PaddedBytes* q, const PaddedBytes* r, const void* matrix, Gaps g, SizeRange s, int32_t x) {
    if (q->kind != kind || r->kind != kind) die("PaddedBytes were built for a different matrix kind");
    const size_t min_size = s.min < 16 ? 16 : s.min, max_size = s.max < 16 ? 16 : s.max;
    std::string why;
    if (check_align_params(false, g, min_size, max_size, x, b->mode, &why)) die("%s", why.c_str());
    if (min_size > max_size) die("min block size exceeds max block size");
    // Allocated::clear (scan_block.rs:1324-1326)
    if (q->len + r->len > b->query_len + b->reference_len) die("sequence lengths exceed the bounds this Block was created with");
    if (max_size > b->max_size) die("max block size exceeds the bound this Block was created with");
    handle_align(b, kind, q->s.data(), q->len, r->s.data(), r->len, nullptr, matrix, g, min_size, max_size, x);
}

static void block_align_profile_impl(BlockImpl* b, const PaddedBytes* q, const AAProfile* pr, SizeRange s, int32_t x) {   // scan_block.rs:942-968
    if (q->kind != BA_KIND_AA) die("PaddedBytes were built for a different matrix kind");
    const size_t min_size = s.min < 16 ? 16 : s.min, max_size = s.max < 16 ? 16 : s.max;
    const Gaps g{0, pr->gap_extend};
    std::string why;
    if (check_align_params(true, g, min_size, max_size, x, b->mode, &why)) die("%s", why.c_str());
    if (min_size > max_size) die("min block size exceeds max block size");
    if (q->len + pr->str_len > b->query_len + b->reference_len) die("sequence lengths exceed the bounds this Block was created with");
    if (max_size > b->max_size) die("max block size exceeds the bound this Block was created with");
    handle_align(b, BA_KIND_PROFILE_, q->s.data(), q->len, nullptr, 0, pr, nullptr, g, min_size, max_size, x);
}

static void block_cigar_impl(BlockImpl* b, bool eq, const PaddedBytes* q, const PaddedBytes* r, size_t i, size_t j, Cigar* cigar) {
    if (!(b->mode & BA_TRACE)) die("trace() requires a Block created with TRACE");   // scan_block.rs:1241-1243
    BaBatch* d = b->dev.get();
    if (!d || !b->aligned) die("cigar requested before any alignment");
    if (eq && d->kind == BA_KIND_PROFILE_) die("cigar_eq needs two sequences; the last alignment was against a profile");
    if (!(i <= b->last_ql && j <= b->last_rl)) die("Traceback cigar end position must be in bounds!");   // scan_block.rs:1483
    if (i + j + 5 > cigar->capacity) die("Cigar was created for shorter sequences than this traceback needs");   // cigar.rs:58-60 slice bound
    (void)q; (void)r;   // the padded images of the aligned pair are already resident on the device
    BatchParams bp = d->params();
    bp.cig_ops = d->cig_ops.as<uint32_t>();
    bp.flags = eq ? (bp.flags | ba::F_CIGAR_EQ) : (bp.flags & ~ba::F_CIGAR_EQ);
    bp.tb_i = (uint32_t)i; bp.tb_j = (uint32_t)j; bp.tb_nblocks = b->last_nblocks; bp.tb_slot = b->last_slot;
    if (hipSetDevice(d->device) != hipSuccess || ba_launch_traceback(d->stream, &bp) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess) die("traceback kernel failed: %s", hipGetErrorString(hipGetLastError()));
    HandleResult hr;
    if (hipMemcpy(&hr, d->rblk.p, sizeof hr, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy D2H failed");
    if (hr.status) die("device traceback failed (status 0x%x)", hr.status);
    const uint32_t n = hr.cig_len;
    std::vector<uint32_t> runs(n);
    if (n && hipMemcpy(runs.data(), d->cig_ops.as<uint32_t>() + (d->cig_total - n), (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
        die("hipMemcpy of cigar runs failed");
    cigar->ops.resize(n);
    for (uint32_t k = 0; k < n; k++) cigar->ops[k] = OpLen{(Operation)(runs[k] & 15), (uintptr_t)(runs[k] >> 4)};
}

// Trace::blocks() (scan_block.rs:1676-1691): the rectangles on the trace stack of the last alignment, in fill order
static size_t block_trace_blocks_impl(BlockImpl* b, Rectangle* out, size_t capacity) {
    if (!(b->mode & BA_TRACE)) die("trace() requires a Block created with TRACE");
    BaBatch* d = b->dev.get();
    if (!d || !b->aligned) die("blocks requested before any alignment");
    const uint32_t nb = b->last_nblocks, slot = b->last_slot;
    if (!out) return nb;
    std::vector<BlockRec> recs(nb);
    if (nb && hipMemcpy(recs.data(), d->blocks.as<BlockRec>() + (size_t)slot * d->blocks_stride, (size_t)nb * sizeof(BlockRec), hipMemcpyDeviceToHost) != hipSuccess)
        die("hipMemcpy of the rectangle list failed");
    for (size_t k = 0; k < nb && k < capacity; k++) out[k] = Rectangle{recs[k].i & 0x7fffffffu, recs[k].j, recs[k].w, recs[k].h};   // (bit 31 of i: trace word layout)
    return nb;
}

extern "C" {

uintptr_t block_trace_blocks_generic(BlockHandle b, Rectangle* out, uintptr_t capacity) { return block_trace_blocks_impl((BlockImpl*)b, out, capacity); }
BlockHandle block_new_generic(uint32_t mode, uintptr_t ql, uintptr_t rl, uintptr_t max_size) { return block_new_impl(mode, ql, rl, max_size); }
void block_align_generic(BlockHandle b, int kind, const PaddedBytes* q, const PaddedBytes* r, const void* matrix, Gaps g, SizeRange s, int32_t x) {
    block_align_impl((BlockImpl*)b, kind, q, r, matrix, g, s, x);
}
void block_align_profile_generic(BlockHandle b, const PaddedBytes* q, const AAProfile* p, SizeRange s, int32_t x) {
    block_align_profile_impl((BlockImpl*)b, q, p, s, x);
}
// The same two calls for a caller that keeps its own PaddedBytes (the Rust crate behind the `simd_hip` feature: rust/src/): the
// padded image as the reference stores it -- [NULL] + converted bytes + NULL padding (scan_block.rs:1790-1812) -- by pointer.
void block_align_padded_generic(BlockHandle bh, int kind, const uint8_t* q_s, uintptr_t q_len, const uint8_t* r_s, uintptr_t r_len, const void* matrix,
                                Gaps g, SizeRange s, int32_t x) {
    BlockImpl* b = (BlockImpl*)bh;
    if (kind < 0 || kind > 2) die("unknown matrix kind %d", kind);
    const size_t min_size = s.min < 16 ? 16 : s.min, max_size = s.max < 16 ? 16 : s.max;
    std::string why;
    if (check_align_params(false, g, min_size, max_size, x, b->mode, &why)) die("%s", why.c_str());
    if (min_size > max_size) die("min block size exceeds max block size");
    if (q_len + r_len > b->query_len + b->reference_len) die("sequence lengths exceed the bounds this Block was created with");
    if (max_size > b->max_size) die("max block size exceeds the bound this Block was created with");
    handle_align(b, kind, q_s, q_len, r_s, r_len, nullptr, matrix, g, min_size, max_size, x);
}
void block_align_profile_padded_generic(BlockHandle bh, const uint8_t* q_s, uintptr_t q_len, const AAProfile* pr, SizeRange s, int32_t x) {
    BlockImpl* b = (BlockImpl*)bh;
    const size_t min_size = s.min < 16 ? 16 : s.min, max_size = s.max < 16 ? 16 : s.max;
    const Gaps g{0, pr->gap_extend};
    std::string why;
    if (check_align_params(true, g, min_size, max_size, x, b->mode, &why)) die("%s", why.c_str());
    if (min_size > max_size) die("min block size exceeds max block size");
    if (q_len + pr->str_len > b->query_len + b->reference_len) die("sequence lengths exceed the bounds this Block was created with");
    if (max_size > b->max_size) die("max block size exceeds the bound this Block was created with");
    handle_align(b, BA_KIND_PROFILE_, q_s, q_len, nullptr, 0, pr, nullptr, g, min_size, max_size, x);
}
AlignResult block_res_generic(BlockHandle b) { return ((BlockImpl*)b)->res; }
void block_cigar_generic(BlockHandle b, uintptr_t i, uintptr_t j, Cigar* c) { block_cigar_impl((BlockImpl*)b, false, nullptr, nullptr, i, j, c); }
void block_cigar_eq_generic(BlockHandle b, const PaddedBytes* q, const PaddedBytes* r, uintptr_t i, uintptr_t j, Cigar* c) {
    block_cigar_impl((BlockImpl*)b, true, q, r, i, j, c);
}
void block_free_generic(BlockHandle b) { delete (BlockImpl*)b; }

#define BA_DEFINE_BLOCK_FNS(S, CIG, CIGEQ, MODE)                                                                                    \
    BlockHandle block_new_##S(uintptr_t ql, uintptr_t rl, uintptr_t max_size) { return block_new_impl(MODE, ql, rl, max_size); }   \
    void block_align_##S(BlockHandle b, const PaddedBytes* q, const PaddedBytes* r, const AAMatrix* m, Gaps g, SizeRange s, int32_t x) { \
        block_align_impl((BlockImpl*)b, BA_KIND_AA, q, r, m, g, s, x);                                                            \
    }                                                                                                                             \
    void block_align_profile_##S(BlockHandle b, const PaddedBytes* q, const AAProfile* p, SizeRange s, int32_t x) {                \
        block_align_profile_impl((BlockImpl*)b, q, p, s, x);                                                                      \
    }                                                                                                                             \
    AlignResult block_res_##S(BlockHandle b) { return ((BlockImpl*)b)->res; }                                                      \
    void CIG(BlockHandle b, uintptr_t i, uintptr_t j, Cigar* c) { block_cigar_impl((BlockImpl*)b, false, nullptr, nullptr, i, j, c); } \
    void CIGEQ(BlockHandle b, const PaddedBytes* q, const PaddedBytes* r, uintptr_t i, uintptr_t j, Cigar* c) {                    \
        block_cigar_impl((BlockImpl*)b, true, q, r, i, j, c);                                                                     \
    }                                                                                                                             \
    void block_free_##S(BlockHandle b) { delete (BlockImpl*)b; }

BA_DEFINE_BLOCK_FNS(aa, _block_cigar_aa, _block_cigar_eq_aa, 0)
BA_DEFINE_BLOCK_FNS(aa_xdrop, _block_cigar_aa_xdrop, _block_cigar_eq_aa_xdrop, BA_X_DROP)
BA_DEFINE_BLOCK_FNS(aa_trace, block_cigar_aa_trace, block_cigar_eq_aa_trace, BA_TRACE)
BA_DEFINE_BLOCK_FNS(aa_trace_xdrop, block_cigar_aa_trace_xdrop, block_cigar_eq_aa_trace_xdrop, BA_TRACE | BA_X_DROP)

}  // extern "C"
