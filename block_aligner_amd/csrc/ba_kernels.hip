// One translation unit per (matrix kind, max-block class): compiled with -DBA_KIND=<0|1|2|3> -DBA_PMAX=<1|2|4|8|16>.
// BA_PMAX = max block size / 128 (packed VGPRs per border array per lane); a smaller class keeps the kernel's VGPR
// budget (and so its occupancy) matched to the batch's max block size.
#include "ba_driver.hpp"
#include "ba_launch.h"

#ifndef BA_KIND
#error "define BA_KIND"
#endif
#ifndef BA_PMAX
#error "define BA_PMAX"
#endif

#ifndef BA_SPECIAL
#define BA_SPECIAL 0   // 1: the kernels of this TU handle LOCAL_START / FREE_QUERY_START_GAPS / FREE_QUERY_END_GAPS batches
#endif

#if !BA_BIG && (BA_KIND != 3 || (!BA_SPECIAL && BA_PMAX <= 8))
#include "ba_multi.hpp"   // (kind 3: k_small's column code builds on multi_rect's helpers; k_multi itself has no profile form)
#endif
#if !BA_BIG && BA_PMAX <= 8 && (BA_KIND != 3 || !BA_SPECIAL)
#include "ba_small.hpp"
#endif
#if !BA_BIG && BA_PMAX == 1 && !BA_SPECIAL
#include "ba_quad.hpp"
#endif
#if BA_KIND == 0 && BA_PMAX == 1 && !BA_SPECIAL && !BA_BIG
#include "ba_seed_device.hpp"   // (k_sort_kat: the sort and the search of the seeding units, for their known-answer test)
#endif

// The catalogue entries of this unit (ba_launch.h): the only place that names a kernel's template arguments and its workgroup size.
// K(T, X) is a family's instantiation with / without traceback and X-drop.
#define K_ALIGN(T, X) ba::k_align<BA_PMAX, BA_KIND, T, X, (BA_SPECIAL != 0)>
#define K_MULTI(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X>
#define K_MULTI_256(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 0, 256>
#define K_MULTI_512(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 0, 512>
#define K_MULTI_G2(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 0, 128, ba::MQ_GEOM_WPW, 2>
#define K_MULTI_G3(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 0, 128, ba::MQ_GEOM_WPW, 3>
#define K_MULTI_S1(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 1>
#define K_MULTI_S2(T, X) ba::k_multi<BA_PMAX, BA_KIND, T, X, 2>
#define K_SMALL(T, X) ba::k_small<BA_PMAX, BA_KIND, T, X>
#define K_SMALL_S1(T, X) ba::k_small<BA_PMAX, BA_KIND, T, X, 1>
#define K_SMALL_S2(T, X) ba::k_small<BA_PMAX, BA_KIND, T, X, 2>
#define K_QUAD(T, X) ba::k_quad<BA_KIND, T, X>
// k_multi's traced kernels for pools beyond 32 bits: P(X) is a family's instantiation of k_multi_p64 with / without X-drop
#define P_MULTI(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X>
#define P_MULTI_256(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 0, 256>
#define P_MULTI_512(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 0, 512>
#define P_MULTI_G2(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 0, 128, ba::MQ_GEOM_WPW, 2>
#define P_MULTI_G3(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 0, 128, ba::MQ_GEOM_WPW, 3>
#define P_MULTI_S1(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 1>
#define P_MULTI_S2(X) ba::k_multi_p64<BA_PMAX, BA_KIND, X, 2>
#define BA_TX(K) {{(const void*)K(false, false), (const void*)K(false, true)}, {(const void*)K(true, false), (const void*)K(true, true)}}
#define BA_PX(P) {(const void*)P(false), (const void*)P(true)}
#define BA_ENTRY(FAM, WPW, K) {FAM, WPW, 0u, {BA_TX(K), {}}, {}}
#define BA_ENTRY_P64(FAM, WPW, K, P) {FAM, WPW, 0u, {BA_TX(K), {}}, {BA_PX(P), {}}}
#define BA_ENTRY_SPM(FAM, WPW, K1, K2, P1, P2) {FAM, WPW, 0u, {BA_TX(K1), BA_TX(K2)}, {BA_PX(P1), BA_PX(P2)}}   // (the batch's flags choose: spm 1 LOCAL_START, spm 2 FREE_QUERY_START_GAPS)

static const ba::KernelEntry g_entries[] = {
    BA_ENTRY(BA_BIG ? ba::FAM_TILED : ba::FAM_PAIR, ba::WAVES_PER_WG, K_ALIGN),
#if BA_KIND != 3 && !BA_SPECIAL && !BA_BIG
    // four pairs per wave while the block is 128 cells, everything else by the same wave on all its lanes (ba_multi.hpp): one kernel per
    // kind and block class
    BA_ENTRY_P64(ba::FAM_MULTI, ba::WAVES_PER_WG, K_MULTI, P_MULTI),
#if BA_KIND == 1 && BA_PMAX >= 4
    // ... with two slots of 256 cells per wave (round 6: DNA batches that start at 256 cells, block classes 512 .. 2048)
    BA_ENTRY_P64(ba::FAM_MULTI_256, ba::WAVES_PER_WG, K_MULTI_256, P_MULTI_256),
#endif
#if BA_KIND == 1 && BA_PMAX >= 8
    // ... with one slot of 512 cells per wave (round 6: DNA batches that start at 512 cells -- percent_len 1 % of reads above 25.6 kbp --, block classes 1024 and 2048)
    BA_ENTRY_P64(ba::FAM_MULTI_512, ba::WAVES_PER_WG, K_MULTI_512, P_MULTI_512),
#endif
#if BA_KIND == 1 && (BA_PMAX == 4 || BA_PMAX == 8)
    // ... in workgroups of four waves at three / two waves per SIMD (round 6: DNA batches whose pairs fill that many waves' slots about once -- ba_host.cpp batch_build)
    BA_ENTRY_P64(ba::FAM_MULTI_G3, ba::MQ_GEOM_WPW, K_MULTI_G3, P_MULTI_G3),
    BA_ENTRY_P64(ba::FAM_MULTI_G2, ba::MQ_GEOM_WPW, K_MULTI_G2, P_MULTI_G2),
#endif
#endif
#if !BA_SPECIAL && !BA_BIG && BA_PMAX <= 8
    // sixteen pairs per wave while the block is 32 cells, everything else by the same wave on all its lanes (ba_small.hpp): one kernel per
    // kind and block class (up to 1024 cells: the solo driver's LDS borders fit in the slots' region)
    BA_ENTRY(ba::FAM_SMALL, ba::WAVES_PER_WG, K_SMALL),
#endif
#if BA_SPECIAL && !BA_BIG && BA_KIND != 3
    // k_multi for LOCAL_START / FREE_QUERY_START_GAPS batches of the sequence kinds: the slots take these modes' plain steps too
    // (FREE_QUERY_END_GAPS batches stay with the per-pair kernel: the mode's running column maxima are not a slot's)
    BA_ENTRY_SPM(ba::FAM_MULTI, ba::WAVES_PER_WG, K_MULTI_S1, K_MULTI_S2, P_MULTI_S1, P_MULTI_S2),
#endif
#if BA_SPECIAL && !BA_BIG && BA_PMAX <= 8 && BA_KIND != 3
    // ... and k_small for the same two modes
    {ba::FAM_SMALL, ba::WAVES_PER_WG, 0u, {BA_TX(K_SMALL_S1), BA_TX(K_SMALL_S2)}, {}},
#endif
#if BA_PMAX == 1 && !BA_SPECIAL && !BA_BIG
    // four pairs per wave while the block is 32 cells (ba_quad.hpp): one kernel per kind, its LDS fixed
    {ba::FAM_QUAD, ba::WAVES_PER_WG, ba::lds_table_bytes_h(BA_KIND) + ba::WAVES_PER_WG * 4 * ba::QUAD_SLOT_BYTES, {BA_TX(K_QUAD), {}}, {}},
#endif
};
[[maybe_unused]] static const int g_registered = ba::register_kernels(BA_KIND, BA_PMAX, BA_SPECIAL != 0, g_entries, (int)(sizeof g_entries / sizeof g_entries[0]));

#if BA_KIND == 0 && BA_PMAX == 1 && !BA_SPECIAL && !BA_BIG
// kernels that exist once
// Traceback from an arbitrary end cell over slot 0's trace (the per-handle API: block_cigar_* after block_align_*).
__global__ void __launch_bounds__(64) k_traceback(const ba::BatchParams bp) {
    using namespace ba;
    __shared__ uint32_t words[4096];
    uint32_t st = 0, n = 0;
    if (bp.flags & (F_LOCAL | F_FQS)) {
        if (lane_id() == 0)
            n = traceback(bp.blocks + (uint64_t)bp.tb_slot * bp.blocks_stride, bp.tb_nblocks, bp.trace_arena + (uint64_t)bp.tb_slot * bp.trace_stride, bp.tb_i,
                          bp.tb_j, bp.pool + bp.q_off[0], bp.pool + bp.r_off[0], bp.flags, bp.cig_ops, bp.cig_off[0], bp.cig_off[1], &st);
    } else
        n = walk_wave<false>(bp.blocks + (uint64_t)bp.tb_slot * bp.blocks_stride, bp.tb_nblocks, bp.trace_arena + (uint64_t)bp.tb_slot * bp.trace_stride, bp.tb_i,
                             bp.tb_j, bp.pool + bp.q_off[0], bp.pool + bp.r_off[0], (bp.flags & F_CIGAR_EQ) != 0, bp.cig_ops, bp.cig_off[0], bp.cig_off[1], &st,
                             words, 4096u);
    if (lane_id() == 0) { bp.cig_len[0] = n; bp.status[0] = st; }
}

// Device-side known-answer test of the lane primitives (round 6; the reference's own: avx2.rs:469-489, plus the carry from vector to vector of
// scan_block.rs:1144-1150): columns of x = D11_open in, R11 out, through the very functions the fill kernels call -- the scan constants
// (make_fill_consts / make_multi_consts / make_small_consts) included. One wave per workgroup; a column starts from MIN = 0 above its first cell.
//   form 0: eight consecutive cells per lane, 16 lanes to a slot (four 128-cell columns per wave): scan8_* + multi_carry (wave_prefix_max16, G / w0).
//           k_multi's order until round 7; no kernel runs this combination any more (k_multi: forms 5 .. 7, scan8_*: form 1) -- it pins multi_carry<16>
//           and w0 against a second, independent in-lane scan
//   form 1: k_small's eight cells per lane, 4 lanes to a slot (sixteen 32-cell columns per wave): scan8_* + small_carry (quad_prefix_max)
//   form 2 / 3 / 4: two cells per lane, 64 / 32 / 16 lanes (one 128- / 64- / 32-cell column per wave): fast_scan (k_align, k_quad, the solo drivers)
//   form 5 / 6 / 7: k_multi's slots as its loop of steps holds them (round 7): eight cells per lane, cells k and k + 4 to a register, 16 / 32 / 64 lanes
//   to a slot (four 128-cell, two 256-cell columns or one 512-cell column per wave): scan_halves + multi_carry<16 / 32 / 64> + apply_halves
// Reached only through the development library (ba_dev_lane_scan, ba_host.cpp).
__global__ void __launch_bounds__(64) k_lane_kat(int form, const short* __restrict__ x, short* __restrict__ out, int gap_extend) {
    using namespace ba;
    const int lane = lane_id();
    if (form >= 5) {
        const short* xi = x + (size_t)blockIdx.x * 512 + lane * 8;
        int r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = pk((int)xi[k], (int)xi[k + 4]);
        const int ge2 = splat(gap_extend);
        const int l = lane & (form == 5 ? 15 : (form == 6 ? 31 : 63));
        const MultiConsts mc = make_multi_consts(l, gap_extend);
        const int r3 = scan_halves(r, ge2, mc);
        const int cs = form == 5 ? multi_carry<16>(r3, mc, l) : (form == 6 ? multi_carry<32>(r3, mc, l) : multi_carry<64>(r3, mc, l));
        apply_halves(r, r3, cs, ge2, mc);
        short* oi = out + (size_t)blockIdx.x * 512 + lane * 8;
#pragma unroll
        for (int k = 0; k < 4; k++) { oi[k] = as_s(r[k]).x; oi[k + 4] = as_s(r[k]).y; }
        return;
    }
    if (form <= 1) {
        const short* xi = x + (size_t)blockIdx.x * 512 + lane * 8;
        int xr[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) xr[k] = pk((int)xi[2 * k], (int)xi[2 * k + 1]);
        const int ge2 = splat(gap_extend);
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = scan8_inreg(xr[k], ge2);
        int G[4], cs;
        if (form == 0) {
            const MultiConsts mc = make_multi_consts(lane & 15, gap_extend);
#pragma unroll
            for (int k = 0; k < 4; k++) G[k] = pk(max(-32768, (2 * k + 1) * gap_extend), max(-32768, (2 * k + 2) * gap_extend));   // what a gap that enters the lane above its first cell has lost on reaching cells 2k, 2k + 1
            scan8_chain(r, G[0]);
            cs = multi_carry(r[3], mc);
        } else {
            const SmallConsts mc = make_small_consts(lane & 3, gap_extend);
#pragma unroll
            for (int k = 0; k < 4; k++) G[k] = mc.G[k];
            scan8_chain(r, G[0]);
            cs = small_carry(r[3], mc, lane & 3);
        }
        short* oi = out + (size_t)blockIdx.x * 512 + lane * 8;
#pragma unroll
        for (int k = 0; k < 4; k++) { const int v = scan8_apply(r[k], cs, G[k], k == 3); oi[2 * k] = as_s(v).x; oi[2 * k + 1] = as_s(v).y; }
    } else {
        const int nl = form == 2 ? 64 : (form == 3 ? 32 : 16);
        const size_t base = (size_t)blockIdx.x * (size_t)(2 * nl);
        const int xv = lane < nl ? pk((int)x[base + 2 * lane], (int)x[base + 2 * lane + 1]) : 0;
        const FillConsts fc = make_fill_consts(lane, 0, gap_extend);
        const int v = form == 2 ? fast_scan<64>(xv, fc) : (form == 3 ? fast_scan<32>(xv, fc) : fast_scan<16>(xv, fc));
        if (lane < nl) { out[base + 2 * lane] = as_s(v).x; out[base + 2 * lane + 1] = as_s(v).y; }
    }
}
extern "C" hipError_t ba_launch_lane_kat(hipStream_t s, int form, const short* x, short* out, int gap_extend, unsigned waves) {
    k_lane_kat<<<dim3(waves), dim3(64), 0, s>>>(form, x, out, gap_extend);
    return hipGetLastError();
}

// Device-side known answers of the single helpers the fill kernels are built from (ba_device.hpp, ba_quad.hpp, ba_multi.hpp, ba_small.hpp, and
// ffbl_u32 of ba_driver.hpp): the lane shifts and broadcasts, the adds and maxima with a fused DPP control, the packed 16-bit arithmetic with its
// op_sel / clamp / SDWA modifiers, the v_perm shuffles, v_bfi, v_cndmask with a scalar mask and the v_writelane parking. One wave per workgroup, all
// 64 lanes active. Lane l of wave w reads four words x[0 .. 3]; k is wave-uniform (a multiplier, a mask, a value to park -- per op). Every operand of
// a helper is a[i] = x[i] ^ (low word of k), computed here: a cross-lane helper then reads a register that a VALU instruction has just written, as
// it does inside the loops of steps, and the wait states between that write and the DPP / swizzle / permute read are the helper's own (the s_nop 1
// inside the assembly strings, the compiler's padding around the builtins). The helpers are called as they stand; templates with the
// instantiations the kernels use plus the edges. op -> helper: the case labels below; tests/lane_prims_ref.py holds the same table and a model of
// every op written from the helper's comment. Four words out per lane; an op leaves the words it does not name at 0.
// Reached only through the development library (ba_dev_lane_prim, ba_host.cpp).
__global__ void __launch_bounds__(64) k_prim_kat(int op, const int4* __restrict__ x, int4* __restrict__ out, unsigned long long k) {
    using namespace ba;
    const int lane = lane_id();
    const size_t at = (size_t)blockIdx.x * 64 + (size_t)lane;
    const int4 xi = x[at];
    const int kl = (int)(uint32_t)k, kh = (int)(uint32_t)(k >> 32);
    int o0 = 0, o1 = 0, o2 = 0, o3 = 0;
#define A0 (xi.x ^ kl)
#define A1 (xi.y ^ kl)
#define A2 (xi.z ^ kl)
#define A3 (xi.w ^ kl)
    switch (op) {
    // ---- shifts
    case 0: o0 = wave_shr1(A0, A1); break;                          // (src, fill)
    case 1: o0 = wave_shr1_z(A0); break;
    case 2: o0 = row_shr1_z(A0); break;
    case 3: o0 = row_shl1_keep(A1, A0); break;                      // (last, src)
    case 4: o0 = quad_shr1(A0); break;
    case 5: o0 = slot_shr1_z<16>(A0, lane & 15); break;
    case 6: o0 = slot_shr1_z<32>(A0, lane & 31); break;
    case 7: o0 = slot_shr1_z<64>(A0, lane); break;
    case 8: o0 = slot_shl1_keep<16>(A1, A0, lane & 15); break;      // (last, src, l)
    case 9: o0 = slot_shl1_keep<32>(A1, A0, lane & 31); break;
    case 10: o0 = slot_shl1_keep<64>(A1, A0, lane); break;
    // ---- broadcasts
    case 11: o0 = row_bcast<0>(A0); break;
    case 12: o0 = row_bcast<15>(A0); break;
    case 13: o0 = row_bcast<7>(A0); break;
    case 14: o0 = slot_bcast<0>(A0); break;
    case 15: o0 = slot_bcast<15>(A0); break;
    case 16: o0 = slot_bcast<3>(A0); break;
    case 17: o0 = quad_bcast<0>(A0); o1 = quad_bcast<1>(A1); o2 = quad_bcast<2>(A2); o3 = quad_bcast<3>(A3); break;
    case 18: o0 = slot_first<16>(A0, lane); break;
    case 19: o0 = slot_first<32>(A0, lane); break;
    case 20: o0 = slot_first<64>(A0, lane); break;
    case 21: o0 = slot_last<16>(A0, lane); break;
    case 22: o0 = slot_last<32>(A0, lane); break;
    case 23: o0 = slot_last<64>(A0, lane); break;
    case 24: o0 = set_lane0(A0, kh); break;
    case 25: { int v = A0; park<0>(v, kh); o0 = v; o1 = unpark<0>(v); break; }
    case 26: { int v = A0; park<31>(v, kh); o0 = v; o1 = unpark<31>(v); break; }
    case 27: { int v = A0; park<63>(v, kh); o0 = v; o1 = unpark<63>(v); break; }
    // ---- adds, maxima and scans over lanes
    case 28: o0 = add_shr1(A0, A1); break;
    case 29: o0 = add_row_shr1(A0, A1); break;
    case 30: o0 = wave_prefix_max(A0); break;
    case 31: o0 = wave_prefix_max16(A0); break;
    case 32: o0 = wave_prefix_max32(A0); break;
    case 33: o0 = max_lanes<16>(A0); break;
    case 34: o0 = max_lanes<32>(A0); break;
    case 35: o0 = max_lanes<64>(A0); break;
    case 36: o0 = wave_max(A0); break;
    case 37: o0 = wave_min(A0); break;
    case 38: first8_max2(A0, A1, o0, o1); break;
    case 39: o0 = quad_prefix_max(A0); break;
    case 40: o0 = quad_all_max(A0); break;
    case 41: case 42: {   // src = (a, ~a), last = (a rotated by one register + 1, by two - 1), the lane mask = k; 41: the first four registers out, 42: the others
        const int sd[4] = {A0, A1, A2, A3}, sr[4] = {~A0, ~A1, ~A2, ~A3};
        const int ld[4] = {A1 + 1, A2 + 1, A3 + 1, A0 + 1}, lr[4] = {A2 - 1, A3 - 1, A0 - 1, A1 - 1};
        int d[4], r[4];
        quad_shl1_keep8(d, r, sd, sr, ld, lr, k);
        if (op == 41) { o0 = d[0]; o1 = d[1]; o2 = d[2]; o3 = d[3]; } else { o0 = r[0]; o1 = r[1]; o2 = r[2]; o3 = r[3]; }
        break;
    }
    // ---- packed and bit arithmetic inside the lane
    case 43: o0 = adds(A0, A1); break;
    case 44: o0 = subs(A0, A1); break;
    case 45: o0 = vmax(A0, A1); break;
    case 46: o0 = vmaxu(A0, A1); break;
    case 47: o0 = neq01(A0, A1, 0x00010001); break;
    case 48: o0 = eq01(A0, A1, 0x00010001); break;
    case 49: o0 = sign_bits(A0); break;
    case 50: o0 = (int)bfi((uint32_t)kh, (uint32_t)A0, (uint32_t)A1); break;
    case 51: o0 = pk_mul(A0, kh); break;
    case 52: o0 = pk_mad(A0, kh, A1); break;
    case 53: o0 = pk_mad_k<2>(A0, A1); break;
    case 54: o0 = pk_mad_k<4>(A0, A1); break;
    case 55: o0 = pk_mad_k<8>(A0, A1); break;
    case 56: o0 = pk_mad_k<0>(A0, A1); break;
    case 57: o0 = pk_mad_k<1>(A0, A1); break;
    case 58: o0 = pk_mad_k<64>(A0, A1); break;
    case 59: o0 = adds_lo(A0, kh); break;
    case 60: o0 = max_hi_lo(A0, A1); break;
    case 61: o0 = splat_lo(A0); break;
    case 62: o0 = splat_hi(A0); break;
    case 63: o0 = scan8_splat_lo(A0); break;
    case 64: o0 = scan8_splat_hi(A0); break;
    case 65: o0 = sel_mask(k, A0, A1); break;
    case 66: { int v[4] = {A0, A1, A2, A3}; cells_split(v); o0 = v[0]; o1 = v[1]; o2 = v[2]; o3 = v[3]; break; }
    case 67: { int v[4] = {A0, A1, A2, A3}; cells_join(v); o0 = v[0]; o1 = v[1]; o2 = v[2]; o3 = v[3]; break; }
    case 68: o0 = clamp16(A0); break;
    case 69: o0 = sat16(A0); break;
    case 70: o0 = (int)ffbl_u32((uint32_t)A0); break;
    case 71: o0 = (int)nuc_col_offsets((uint32_t)A0); break;
    case 72: o0 = (int)nuc_keys2((uint32_t)A0); break;
    case 73: o0 = (int)add_word((uint32_t)A0, (uint32_t)A1, 0); o1 = (int)add_word((uint32_t)A0, (uint32_t)A1, 1); break;
    case 74: o0 = (int)add_byte((uint32_t)A0, (uint32_t)A1, 0); o1 = (int)add_byte((uint32_t)A0, (uint32_t)A1, 1);
             o2 = (int)add_byte((uint32_t)A0, (uint32_t)A1, 2); o3 = (int)add_byte((uint32_t)A0, (uint32_t)A1, 3); break;
    case 75: o0 = pk(A0, A1); break;
    case 76: o0 = splat(A0); break;
    case 77: o0 = scan8_inreg(A0, kh); break;
    default: break;
    }
#undef A0
#undef A1
#undef A2
#undef A3
    out[at] = int4{o0, o1, o2, o3};
}
extern "C" hipError_t ba_launch_prim_kat(hipStream_t s, int op, const int* x, int* out, unsigned long long k, unsigned waves) {
    k_prim_kat<<<dim3(waves), dim3(64), 0, s>>>(op, (const int4*)x, (int4*)out, k);
    return hipGetLastError();
}

// ... and of the normalized bitonic network and the binary search that seeding, the reference index and the selection share (ba_seed_device.hpp):
// one workgroup of THREADS threads sorts keys[0 .. n) in LDS, n <= CAP, as k_seeding_sort / k_index_hit_sort (1024 threads, SEEDING_SORT_LDS keys)
// and k_select_mark (64 threads, SELECT_MAX_PER_READ keys) do; lb[i] = lower_bound of the caller's i-th key in the sorted array.
template <uint32_t THREADS, uint32_t CAP>
__global__ void __launch_bounds__(THREADS) k_sort_kat(uint64_t* keys, uint32_t n, uint32_t* lb) {
    __shared__ uint64_t sorted[CAP];
    if (n > CAP) return;
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) sorted[i] = keys[i];
    __syncthreads();
    ba::seed::sort_network<THREADS>(sorted, n);
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) lb[i] = ba::seed::lower_bound(sorted, n, keys[i]);
    __syncthreads();   // (every thread has read the caller's keys)
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) keys[i] = sorted[i];
}
extern "C" hipError_t ba_launch_sort_kat(hipStream_t s, int threads, uint64_t* keys, uint32_t n, uint32_t* lb) {
    if (threads == 64) k_sort_kat<64, ba::SELECT_MAX_PER_READ><<<dim3(1), dim3(64), 0, s>>>(keys, n, lb);
    else k_sort_kat<1024, ba::SEEDING_SORT_LDS><<<dim3(1), dim3(1024), 0, s>>>(keys, n, lb);
    return hipGetLastError();
}

// Pair-slot batches: all tracebacks of the batch, one pair per lane (ba_driver.hpp traceback_all).
constexpr int WALK_WAVES = 4;
__global__ void __launch_bounds__(WALK_WAVES * 64) k_walk(const ba::BatchParams bp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char walk_lds[];
    ba::traceback_all(bp, (uint32_t)ba::F_CIGAR_EQ, walk_lds + ((uint32_t)threadIdx.x >> 6) * ba::TB_LDS_BYTES);
}

// ... of a k_small batch (slot rectangles: words of 4 cells x 2 columns; the lanes' records are larger)
__global__ void __launch_bounds__(WALK_WAVES * 64) k_walk_l2(const ba::BatchParams bp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char walk_lds[];
    ba::traceback_all<true>(bp, (uint32_t)ba::F_CIGAR_EQ, walk_lds + ((uint32_t)threadIdx.x >> 6) * ba::TB_LDS_BYTES_L2);
}

// ... of a LOCAL_START / FREE_QUERY_START_GAPS batch of k_small (the lanes' records also hold the cells' zero-mask bits)
__global__ void __launch_bounds__(WALK_WAVES * 64) k_walk_loc(const ba::BatchParams bp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char walk_lds[];
    ba::traceback_all<true, true>(bp, (uint32_t)ba::F_CIGAR_EQ, walk_lds + ((uint32_t)threadIdx.x >> 6) * ba::TB_LDS_BYTES_LOC);
}

__global__ void __launch_bounds__(256) k_compact_cigars(const uint32_t* __restrict__ ops, const uint64_t* __restrict__ cig_off,
                                                        const uint32_t* __restrict__ cig_len, const uint64_t* __restrict__ out_off,
                                                        uint32_t* __restrict__ out, uint32_t n) {
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const uint32_t len = cig_len[p];
        const uint64_t src = cig_off[p + 1] - len, dst = out_off[p];
        for (uint32_t k = threadIdx.x; k < len; k += blockDim.x) out[dst + k] = ops[src + k];
    }
}
// Offsets of the compacted CIGAR runs, pair after pair in the CALLER's order (dev_of[p] = device position of the caller's pair p):
// out_off[dev_of[p]] = sum of cig_len[dev_of[p']] over p' < p; *total = the sum over all pairs. One workgroup: per-thread chunk sums,
// a scan over the 1024 partial sums, a second pass.
__global__ void __launch_bounds__(1024) k_cigar_offsets(const uint32_t* __restrict__ cig_len, const uint32_t* __restrict__ dev_of, uint64_t* __restrict__ out_off,
                                                        unsigned long long* __restrict__ total, uint32_t n) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (uint32_t p = lo; p < hi; p++) sum += cig_len[dev_of ? dev_of[p] : p];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive scan
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long at = part[t] - sum;
    for (uint32_t p = lo; p < hi; p++) { const uint32_t s = dev_of ? dev_of[p] : p; out_off[s] = at; at += cig_len[s]; }
    if (t == 1023) *total = part[1023];
}
// the gather itself, only if everything fits (else *total says how much is needed and nothing is written)
__global__ void __launch_bounds__(256) k_compact_cigars_checked(const uint32_t* __restrict__ ops, const uint64_t* __restrict__ cig_off,
                                                                const uint32_t* __restrict__ cig_len, const uint64_t* __restrict__ out_off,
                                                                uint32_t* __restrict__ out, uint32_t n, const unsigned long long* __restrict__ total, unsigned long long capacity) {
    if (*total > capacity) return;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const uint32_t len = cig_len[p];
        const uint64_t src = cig_off[p + 1] - len, dst = out_off[p];
        for (uint32_t k = threadIdx.x; k < len; k += blockDim.x) out[dst + k] = ops[src + k];
    }
}
extern "C" hipError_t ba_launch_cigar_offsets_and_compact(hipStream_t s, const uint32_t* ops, const uint64_t* cig_off, const uint32_t* cig_len, const uint32_t* dev_of,
                                                          uint64_t* out_off, uint32_t* out, unsigned long long* total, unsigned long long capacity, uint32_t n) {
    k_cigar_offsets<<<dim3(1), dim3(1024), 0, s>>>(cig_len, dev_of, out_off, total, n);
    const unsigned grid = n < 4096 ? (n ? n : 1) : 4096;
    k_compact_cigars_checked<<<dim3(grid), dim3(256), 0, s>>>(ops, cig_off, cig_len, out_off, out, n, total, capacity);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_compact_cigars(hipStream_t s, const uint32_t* ops, const uint64_t* cig_off, const uint32_t* cig_len,
                                               const uint64_t* out_off, uint32_t* out, uint32_t n) {
    const unsigned grid = n < 4096 ? (n ? n : 1) : 4096;
    k_compact_cigars<<<dim3(grid), dim3(256), 0, s>>>(ops, cig_off, cig_len, out_off, out, n);
    return hipGetLastError();
}
// PaddedBytes images on the device (scan_block.rs:1798-1850: [NULL] + convert(bytes) + NULL padding; convert_char of
// scores.rs:130-134 / 212-216 / 270-272): one workgroup per sequence, four image bytes per thread and store. A byte the
// reference would assert on is reported through *err (lowest pair wins): pair << 8 | byte.
__global__ void __launch_bounds__(256) k_pack_sequences(int kind, const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_q,
                                                        const uint64_t* __restrict__ raw_r, const uint64_t* __restrict__ q_off,
                                                        const uint32_t* __restrict__ q_len, const uint64_t* __restrict__ r_off,
                                                        const uint32_t* __restrict__ r_len, uint8_t* __restrict__ image, uint32_t pad,
                                                        unsigned long long* err) {
    const uint32_t p = blockIdx.x >> 1;
    const bool ref = blockIdx.x & 1;
    const uint8_t* src = raw + (ref ? raw_r[p] : raw_q[p]);
    const uint32_t len = ref ? r_len[p] : q_len[p];
    uint32_t* dst = (uint32_t*)(image + (ref ? r_off[p] : q_off[p]));   // images start 4-byte aligned
    const uint32_t null_b = kind == ba::KIND_AA ? 26u : (kind == ba::KIND_NUC ? (uint32_t)'Z' : 0u);
    const uint32_t words = ((1u + len + pad + 3u) & ~3u) / 4u;
    for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) {
        uint32_t wd = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t pos = 4 * k + b;
            uint32_t c = null_b;
            if (pos >= 1 && pos <= len) {
                c = src[pos - 1];
                if (kind != ba::KIND_BYTES) {
                    if (c >= 'a' && c <= 'z') c -= 32;
                    const bool ok = kind == ba::KIND_AA ? (c >= 'A' && c <= 'A' + 26) : (c >= 'A' && c <= 'Z');
                    if (!ok) { atomicMin(err, ((unsigned long long)p << 8) | src[pos - 1]); c = null_b; }
                    else if (kind == ba::KIND_AA) c -= 'A';
                }
            }
            wd |= c << (8 * b);
        }
        dst[k] = wd;
    }
}
extern "C" hipError_t ba_launch_pack_sequences(hipStream_t s, int kind, const uint8_t* raw, const uint64_t* raw_q, const uint64_t* raw_r,
                                               const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                               uint8_t* image, uint32_t pad, uint32_t n, unsigned long long* err) {
    k_pack_sequences<<<dim3(2 * n), dim3(256), 0, s>>>(kind, raw, raw_q, raw_r, q_off, q_len, r_off, r_len, image, pad, err);
    return hipGetLastError();
}
// Results of a re-run (pairs whose trace stack outgrew an adaptively sized slot, see batch_plan) back into the batch's own
// arrays: one workgroup per pair; sub-batch entry k belongs to the batch's (device-order) pair idx[k].
__global__ void __launch_bounds__(256) k_merge_retry(const uint32_t* __restrict__ idx, const ba::BatchParams sub, const ba::BatchParams dst,
                                                     const uint32_t* __restrict__ sub_trace_words, uint32_t* __restrict__ dst_trace_words) {
    const uint32_t k = blockIdx.x, p = idx[k];
    const uint32_t len = sub.cig_len[k];
    if (threadIdx.x == 0) {
        dst.score[p] = sub.score[k]; dst.query_idx[p] = sub.query_idx[k]; dst.reference_idx[p] = sub.reference_idx[k];
        dst.cig_len[p] = len; dst.status[p] = sub.status[k]; dst.cells[p] = sub.cells[k];
        dst_trace_words[p] = sub_trace_words[k];
    }
    if (!sub.cig_ops || !dst.cig_ops) return;
    const uint64_t src = sub.cig_off[k + 1] - len, to = dst.cig_off[p + 1] - len;   // runs are right-aligned in a pair's range
    for (uint32_t t = threadIdx.x; t < len; t += blockDim.x) dst.cig_ops[to + t] = sub.cig_ops[src + t];
}
extern "C" hipError_t ba_launch_merge_retry(hipStream_t s, const uint32_t* idx, uint32_t k, const ba::BatchParams* sub, const ba::BatchParams* dst,
                                            const uint32_t* sub_tw, uint32_t* dst_tw) {
    k_merge_retry<<<dim3(k), dim3(256), 0, s>>>(idx, *sub, *dst, sub_tw, dst_tw);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_walk(hipStream_t s, const ba::BatchParams* bp, uint32_t grid) {
    k_walk<<<dim3(grid), dim3(WALK_WAVES * 64), WALK_WAVES * ba::TB_LDS_BYTES, s>>>(*bp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_walk_l2(hipStream_t s, const ba::BatchParams* bp, uint32_t grid) {
    k_walk_l2<<<dim3(grid), dim3(WALK_WAVES * 64), WALK_WAVES * ba::TB_LDS_BYTES_L2, s>>>(*bp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_walk_loc(hipStream_t s, const ba::BatchParams* bp, uint32_t grid) {
    k_walk_loc<<<dim3(grid), dim3(WALK_WAVES * 64), WALK_WAVES * ba::TB_LDS_BYTES_LOC, s>>>(*bp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_traceback(hipStream_t s, const ba::BatchParams* bp) {
    k_traceback<<<dim3(1), dim3(64), 0, s>>>(*bp);
    return hipGetLastError();
}
#endif
