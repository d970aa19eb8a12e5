// Per-alignment statistics (ba_*_stats, ba_host.cpp): identity, edits, gaps and the start cell of every traced alignment, computed from the
// batch's CIGAR runs and sequence images where the fill left them. No fill kernel is touched.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

constexpr uint32_t STATS_WAVES = 4;   // waves per workgroup of k_stats

// one wave's LDS operations execute in program order; this only keeps the compiler from reordering them across a hand-off between lanes
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= (uint32_t)d ? o : 0u;
    }
    return x;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, d, 64));
    return x;
}

// the fill's score of image byte a (query) against image byte b (reference); indices clamped into the table
__device__ __forceinline__ int cell_score(int kind, const int8_t* m, uint32_t a, uint32_t b) {
    if (kind == ba::KIND_NUC) return m[(a & 7u) * 16u + (b & 15u)];
    if (kind == ba::KIND_AA) return m[min(a, 26u) * 32u + min(b, 31u)];
    return a == b ? m[0] : m[1];
}

}  // namespace

// One wave per pair, pairs in the batch's device order (longest first), grid-stride. The runs are read 64 at a time from the last one back:
// the pair's end cell is known, so a wave-wide prefix sum of what every run consumes gives every run its first cell, and after the last chunk
// the running position is the path's start. The match-type cells of a chunk are spread over the lanes (cell t of the chunk to lane t % 64),
// so a long M run is read by the whole wave: each lane finds its cell's run in the chunk's table in LDS, reads both image bytes and scores
// them from the matrix in LDS. Per-lane sums and maxima are reduced across the wave once per pair; lane 0 writes the record.
__global__ void __launch_bounds__(256) k_stats(const ba::StatsParams sp) {
    __shared__ int8_t tab[1024];
    // per wave, the chunk's runs: match-type cells of the runs up to and including run k; its first cell's i and j, less the match-type
    // cells before it (cell t of the chunk, in run k, lies at i = iadj[k] + t, j = jadj[k] + t)
    __shared__ uint32_t chunk[STATS_WAVES][3][64];
    for (uint32_t k = threadIdx.x; k < sp.matrix_bytes && k < 1024u; k += blockDim.x) tab[k] = sp.matrix[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t* incl = chunk[w][0];
    uint32_t* iadj = chunk[w][1];
    uint32_t* jadj = chunk[w][2];
    for (uint32_t d = blockIdx.x * STATS_WAVES + w; d < sp.n; d += gridDim.x * STATS_WAVES) {
        const bool failed = (sp.status[d] & ba::STATS_FAILED) != 0;
        const uint32_t nrun = failed ? 0u : sp.cig_len[d];
        uint32_t ci = failed ? 0u : sp.qidx[d], cj = failed ? 0u : sp.ridx[d];   // end of the chunk being read = start of the one after it
        const uint32_t ql = sp.q_len[d], rl = sp.r_len[d];
        const uint8_t* q = sp.pool + sp.q_off[d] + 1;
        const uint8_t* r = sp.pool + sp.r_off[d] + 1;
        const uint32_t* ops = sp.cig_ops + (sp.cig_off[d + 1] - nrun);
        uint32_t cols = 0, mat = 0, mis = 0, pos = 0, ins = 0, del = 0, opens = 0, lins = 0, ldel = 0;
        int score = 0;
        bool bad = false;   // runs that consume more than the end cell or leave a sequence: no record (never for the library's own runs)
        for (uint32_t hi = nrun; hi > 0;) {
            const uint32_t lo = hi > 64u ? hi - 64u : 0u, cnt = hi - lo;
            const uint32_t x = lane < cnt ? ops[lo + lane] : 0u;
            const uint32_t op = x & 15u, len = x >> 4;
            const bool m = op >= 1u && op <= 3u, gi = op == 4u, gd = op == 5u;
            const uint32_t cq = (m || gi) ? len : 0u, cr = (m || gd) ? len : 0u, cm = m ? len : 0u;
            const uint32_t sq = wave_incl_sum(cq, lane), sr = wave_incl_sum(cr, lane), sm = wave_incl_sum(cm, lane);
            const uint32_t tq = (uint32_t)__shfl((int)sq, 63, 64), tr = (uint32_t)__shfl((int)sr, 63, 64), tm = (uint32_t)__shfl((int)sm, 63, 64);
            bad = bad || tq > ci || tr > cj;
            // run k ends where the runs after it in the chunk begin; its first cell is that less what it consumes
            const uint32_t i0 = ci - (tq - sq) - cq, j0 = cj - (tr - sr) - cr;
            cols += len;
            if (gi || gd) {
                opens++;
                score += sp.gap_open + (int)(len - 1u) * sp.gap_extend;
                if (gi) { ins += len; lins = max(lins, len); } else { del += len; ldel = max(ldel, len); }
            }
            incl[lane] = sm; iadj[lane] = i0 - (sm - cm); jadj[lane] = j0 - (sm - cm);
            wave_lds_fence();
            if (!bad) {
                uint32_t k = 0, kend = incl[0], ia = iadj[0], ja = jadj[0];
                for (uint32_t t = lane; t < tm; t += 64u) {
                    if (t >= kend) {
                        do k++; while (incl[k] <= t);   // (t < tm = incl[63]: ends inside the chunk)
                        kend = incl[k]; ia = iadj[k]; ja = jadj[k];
                    }
                    const uint32_t i = ia + t, j = ja + t;
                    if (i >= ql || j >= rl) { bad = true; break; }
                    const uint32_t a = q[i], b = r[j];
                    const int s = cell_score(sp.kind, tab, a, b);
                    mat += a == b; mis += a != b; pos += s > 0; score += s;
                }
            }
            wave_lds_fence();   // (the next chunk overwrites the table)
            ci -= tq; cj -= tr;
            hi = lo;
        }
        bad = __any(bad);
        ba::AlignStats o;
        o.q_start = ci; o.r_start = cj;
        o.columns = wave_sum(cols); o.matches = wave_sum(mat); o.mismatches = wave_sum(mis); o.positives = wave_sum(pos);
        o.ins = wave_sum(ins); o.del = wave_sum(del); o.gap_opens = wave_sum(opens);
        o.longest_ins = wave_max(lins); o.longest_del = wave_max(ldel);
        o.path_score = (int32_t)wave_sum((uint32_t)score);
        if (bad) o = ba::AlignStats{};
        if (lane == 0) sp.out[sp.out_pos ? sp.out_pos[d] : d] = o;
    }
}

// Extension batches: one thread per seed. The seed's record = its left side's record (the inner batch's, by device position) + the seed's
// ungapped columns (read from seed_pool, as the splice reads them) + its right side's record: counts add, the longest gaps take the maximum,
// the start is the extension's. Exact, because the splice's joins only merge match-type runs: every gap run of the spliced CIGAR is one
// side's. A seed whose status has a failure bit gets an all-zero record.
__global__ void __launch_bounds__(256) k_stats_extend(const ba::ExtendParams ep, const ba::AlignStats* __restrict__ side, ba::AlignStats* __restrict__ out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ep.n) return;
    ba::AlignStats o{};
    if (!(ep.status[s] & ba::STATS_FAILED)) {
        const uint32_t L = ep.seed_len[s];
        const uint8_t* qs = ep.seed_pool + ep.seed_q[s] + 1;
        const uint8_t* rs = ep.seed_pool + ep.seed_r[s] + 1;
        int sc = 0;
        for (uint32_t k = 0; k < L; k++) {
            const uint32_t a = qs[k], b = rs[k];
            const int x = cell_score(ep.kind, ep.matrix, a, b);
            sc += x; o.matches += a == b; o.mismatches += a != b; o.positives += x > 0;
        }
        o.columns = L; o.path_score = sc;
        const uint32_t dl = ep.side[2 * s], dr = ep.side[2 * s + 1];
        for (const uint32_t dd : {dl, dr}) {
            if (dd == ba::EXT_NO_SIDE) continue;
            const ba::AlignStats x = side[dd];
            o.columns += x.columns; o.matches += x.matches; o.mismatches += x.mismatches; o.positives += x.positives;
            o.ins += x.ins; o.del += x.del; o.gap_opens += x.gap_opens; o.path_score += x.path_score;
            o.longest_ins = max(o.longest_ins, x.longest_ins); o.longest_del = max(o.longest_del, x.longest_del);
        }
        o.q_start = ep.q_seed[s] - (dl != ba::EXT_NO_SIDE ? ep.in_qidx[dl] : 0u);
        o.r_start = ep.r_seed[s] - (dl != ba::EXT_NO_SIDE ? ep.in_ridx[dl] : 0u);
    }
    out[s] = o;
}

namespace {
__device__ __forceinline__ void add_record(const ba::AlignStats& x, uint32_t& cols, uint32_t& mat, uint32_t& mis, uint32_t& pos, uint32_t& ins, uint32_t& del,
                                           uint32_t& opens, uint32_t& lins, uint32_t& ldel, int& score) {
    cols += x.columns; mat += x.matches; mis += x.mismatches; pos += x.positives; ins += x.ins; del += x.del; opens += x.gap_opens;
    lins = max(lins, x.longest_ins); ldel = max(ldel, x.longest_del); score += x.path_score;
}
}  // namespace

// Chain batches: one wave per chain at a time, chains in the caller's order, grid-stride. The chain's record = the sum over its 2 K + 1
// elements (ba_chain.h): the ends' and the aligned gaps' records (the inner batches', by device position) as they are -- counts do not depend
// on the reversal of the left end --, every anchor's ungapped columns scored from anchor_pool, every gap with one empty slice one I or D run of
// its length d (one gap open, open + (d - 1) * extend). Counts add, the longest gaps take the maximum, the start is the first anchor's less
// what the left end consumed. Exact: every gap element lies between two anchors and an anchor always has match-type runs, so a gap run of one
// element never merges with a gap run of another (the splice's joins only lengthen runs whose counts add anyway: INTEGRATION.md, "Anchor
// chains"; tests/chain_ref.py asserts gap_merges == 0) -- the number and the lengths of the spliced CIGAR's gap runs are the elements' own.
// The lanes stride over the anchors 64 at a time, each with the gap behind its anchor; the chunk's columns are spread over the lanes as
// k_stats spreads a long M run (a prefix sum of anchor_len, column t of the chunk to lane t % 64), so that a long anchor is read by the whole
// wave. A chain whose status has a failure bit gets an all-zero record.
__global__ void __launch_bounds__(64 * STATS_WAVES) k_stats_chain(const ba::ChainParams cp, const ba::AlignStats* __restrict__ ends,
                                                                  const ba::AlignStats* __restrict__ gaps, ba::AlignStats* __restrict__ out) {
    __shared__ int8_t tab[1024];
    // per wave, the chunk's anchors: columns of the anchors up to and including anchor k; its images' first bytes in anchor_pool, less the
    // columns before it (column t of the chunk, in anchor k, is qadj[k] + t against radj[k] + t)
    __shared__ uint32_t incl_s[STATS_WAVES][64];
    __shared__ uint64_t qadj_s[STATS_WAVES][64], radj_s[STATS_WAVES][64];
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = cp.matrix[k];   // (the matrix buffer of a spliced batch is 1024 bytes)
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t* incl = incl_s[w];
    uint64_t* qadj = qadj_s[w];
    uint64_t* radj = radj_s[w];
    for (uint32_t c = blockIdx.x * STATS_WAVES + w; c < cp.n; c += gridDim.x * STATS_WAVES) {
        const uint64_t a0 = cp.anchor_first[c];
        const uint32_t K = (uint32_t)(cp.anchor_first[c + 1] - a0);
        const uint32_t dl = cp.end_side[2 * c], dr = cp.end_side[2 * c + 1];
        const bool failed = (cp.status[c] & ba::STATS_FAILED) != 0;
        uint32_t cols = 0, mat = 0, mis = 0, pos = 0, ins = 0, del = 0, opens = 0, lins = 0, ldel = 0;
        int score = 0;
        if (!failed) {
            if (lane == 0 && dl != ba::CHAIN_NO_PIECE) add_record(ends[dl], cols, mat, mis, pos, ins, del, opens, lins, ldel, score);
            if (lane == 1 && dr != ba::CHAIN_NO_PIECE) add_record(ends[dr], cols, mat, mis, pos, ins, del, opens, lins, ldel, score);
        }
        for (uint32_t base = 0; base < K && !failed; base += 64u) {
            const uint32_t k = base + lane;
            const bool in = k < K;
            const uint64_t a = a0 + k;
            const uint32_t L = in ? cp.anchor_len[a] : 0u;
            if (in && k + 1 < K) {   // the gap behind the anchor
                const uint32_t d = cp.gap_side[a];
                if (d != ba::CHAIN_NO_PIECE) add_record(gaps[d], cols, mat, mis, pos, ins, del, opens, lins, ldel, score);
                else {
                    const uint32_t dq = cp.q_anchor[a + 1] - cp.q_anchor[a] - L, dd = cp.r_anchor[a + 1] - cp.r_anchor[a] - L;   // (one of them is 0)
                    const uint32_t len = dq | dd;
                    if (len) {
                        cols += len; opens++;
                        score += cp.gap_open + (int)(len - 1u) * cp.gap_extend;
                        if (dq) { ins += len; lins = max(lins, len); } else { del += len; ldel = max(ldel, len); }
                    }
                }
            }
            // the anchors of a chain are disjoint on the query: the columns of a chunk are fewer than 2^32
            const uint32_t sm = wave_incl_sum(L, lane), tm = (uint32_t)__shfl((int)sm, 63, 64);
            incl[lane] = sm;
            qadj[lane] = in ? cp.anchor_q[a] + 1 - (sm - L) : 0u;
            radj[lane] = in ? cp.anchor_r[a] + 1 - (sm - L) : 0u;
            wave_lds_fence();
            {
                uint32_t j = 0, jend = incl[0];
                uint64_t qa = qadj[0], ra = radj[0];
                for (uint32_t t = lane; t < tm; t += 64u) {
                    if (t >= jend) {
                        do j++; while (incl[j] <= t);   // (t < tm = incl[63]: ends inside the chunk)
                        jend = incl[j]; qa = qadj[j]; ra = radj[j];
                    }
                    const uint32_t x = cp.anchor_pool[qa + t], y = cp.anchor_pool[ra + t];
                    const int s = cell_score(cp.kind, tab, x, y);
                    mat += x == y; mis += x != y; pos += s > 0; score += s;
                }
            }
            cols += L;
            wave_lds_fence();   // (the next chunk overwrites the table)
        }
        ba::AlignStats o{};
        o.columns = wave_sum(cols); o.matches = wave_sum(mat); o.mismatches = wave_sum(mis); o.positives = wave_sum(pos);
        o.ins = wave_sum(ins); o.del = wave_sum(del); o.gap_opens = wave_sum(opens);
        o.longest_ins = wave_max(lins); o.longest_del = wave_max(ldel);
        o.path_score = (int32_t)wave_sum((uint32_t)score);
        if (!failed) {
            o.q_start = cp.q_anchor[a0] - (dl != ba::CHAIN_NO_PIECE ? cp.ends.qidx[dl] : 0u);
            o.r_start = cp.r_anchor[a0] - (dl != ba::CHAIN_NO_PIECE ? cp.ends.ridx[dl] : 0u);
        }
        if (lane == 0) out[c] = o;
    }
}

extern "C" hipError_t ba_launch_stats(hipStream_t s, const ba::StatsParams* sp) {
    if (!sp->n) return hipSuccess;
    const uint32_t wgs = (sp->n + STATS_WAVES - 1) / STATS_WAVES;
    k_stats<<<dim3(wgs < 2048u ? wgs : 2048u), dim3(64 * STATS_WAVES), 0, s>>>(*sp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_stats_extend(hipStream_t s, const ba::ExtendParams* ep, const ba::AlignStats* side, ba::AlignStats* out) {
    if (!ep->n) return hipSuccess;
    k_stats_extend<<<dim3((ep->n + 255) / 256), dim3(256), 0, s>>>(*ep, side, out);
    return hipGetLastError();
}
// ends / gaps: the inner batches' records in their device order; null for a set without such pieces
extern "C" hipError_t ba_launch_stats_chain(hipStream_t s, const ba::ChainParams* cp, const ba::AlignStats* ends, const ba::AlignStats* gaps,
                                            ba::AlignStats* out) {
    if (!cp->n) return hipSuccess;
    const uint32_t wgs = (cp->n + STATS_WAVES - 1) / STATS_WAVES;
    k_stats_chain<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * STATS_WAVES), 0, s>>>(*cp, ends, gaps, out);
    return hipGetLastError();
}
