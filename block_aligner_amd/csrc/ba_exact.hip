// Exact full-matrix scores (ba_*_exact, ba_host.cpp): textbook Gotoh H / E / F over the whole |q| x |r| matrix of a pair, in int32, from
// the batch's sequence images, matrix and gaps. No alignment kernel is touched; nothing of a run is read.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

constexpr int NEG = ba::EXACT_NEG;

// lane l <- lane l - 1 across the whole wave; lane 0 keeps `first`
__device__ __forceinline__ int wave_shr1_first(int src, int first) { return __builtin_amdgcn_update_dpp(first, src, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int wave_max_i(int x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = max(x, __shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ int wave_incl_max(int x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(x, d, 64);
        x = lane >= (uint32_t)d ? max(x, o) : x;
    }
    return x;
}

// The fill's score of image byte a (query) against image byte b (reference), split in two: what depends on a alone (once per band and
// lane), what depends on b alone (once per 64 columns), and the table read per cell.
template <int KIND> __device__ __forceinline__ uint32_t q_part(uint32_t a) {
    if constexpr (KIND == ba::KIND_NUC) return (a & 7u) * 16u;
    else if constexpr (KIND == ba::KIND_AA) return min(a, 26u) * 32u;
    else return a;
}
template <int KIND> __device__ __forceinline__ uint32_t r_part(uint32_t b) {
    if constexpr (KIND == ba::KIND_NUC) return b & 15u;
    else if constexpr (KIND == ba::KIND_AA) return min(b, 31u);
    else return b;
}
template <int KIND> __device__ __forceinline__ int cell_score(const int8_t* tab, uint32_t qa, uint32_t rb) {
    if constexpr (KIND == ba::KIND_BYTES) return qa == rb ? tab[0] : tab[1];
    else return tab[qa + rb];
}

// One pair on one wave. Rows are query positions, columns reference positions. A band is 64 rows, lane l owns row i0 + l + 1 and walks it
// left to right, one column per step, skewed: at step t lane l is at column t - l + 1. H and the vertical-gap state V of the row above
// come down one lane per step (DPP wave shift); the horizontal-gap state and the diagonal stay in the lane. Lane 0's row above is the
// last row of the band before, which lane 63 left in the wave's row buffer -- or row 0, which is computed. Both ends of the buffer
// traffic go through registers 64 columns at a time (one coalesced load / store per 64 steps, a v_readlane and a select per step); the
// same holds for the reference bytes. Every lane keeps its row's maximum and first argmax; after a band they are examined in row order.
template <int KIND>
__device__ void exact_pair(const ba::ExactParams& xp, const int8_t* tab, int2* rowbuf, uint32_t lane, uint32_t d, ba::Exact* out) {
    const uint32_t ql = xp.q_len[d], rl = xp.r_len[d];
    const uint8_t* q = xp.pool + xp.q_off[d] + 1;
    const uint8_t* r = xp.pool + xp.r_off[d] + 1;
    const int go = xp.gap_open, ge = xp.gap_extend;
    const bool extend = xp.what == ba::EXACT_EXTEND, xdrop = extend && xp.x_drop >= 0;
    int best = 0; uint32_t bi = 0, bj = 0;                 // EXTEND: cell (0, 0) = 0 is the maximum of row 0 (gap costs are negative)
    uint32_t rows = ql + 1;
    int corner = rl ? go + (int)(rl - 1) * ge : 0;         // GLOBAL: H[|q|][|r|]; this is row 0's
    bool stopped = false;
    for (uint32_t i0 = 0; i0 < ql && !stopped; i0 += ba::EXACT_BAND) {
        const uint32_t nb = min(ba::EXACT_BAND, ql - i0);
        const bool first = i0 == 0, last = i0 + ba::EXACT_BAND >= ql;
        const uint32_t i = i0 + lane + 1;
        const bool rowok = lane < nb;
        const uint32_t qa = q_part<KIND>(rowok ? q[i - 1] : 0u);
        int Hcur = go + (int)(i - 1) * ge;                 // H[i][0]
        int diag = i == 1 ? 0 : go + (int)(i - 2) * ge;    // H[i - 1][0]
        int Hz = NEG, Vcur = NEG;                          // no gap ends in column 0
        int rmax = Hcur; uint32_t rj = 0;
        int inH = NEG, inV = NEG, outH = 0, outV = 0;
        uint32_t rch = 0, b = 0;
        const uint32_t T = rl ? rl + nb - 1 : 0;
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t c = t & 63u;
            if (c == 0) {   // the next 64 columns of the row above and of the reference: lane k holds column t + 1 + k
                const uint32_t jc = t + 1 + lane;
                const bool in = jc <= rl;
                if (first) { inH = go + (int)(jc - 1) * ge; inV = NEG; }
                else { const int2 x = in ? rowbuf[jc] : make_int2(NEG, NEG); inH = x.x; inV = x.y; }
                rch = r_part<KIND>(in ? r[jc - 1] : 0u);
            }
            const int upH = wave_shr1_first(Hcur, __builtin_amdgcn_readlane(inH, c));
            const int upV = wave_shr1_first(Vcur, __builtin_amdgcn_readlane(inV, c));
            b = (uint32_t)wave_shr1_first((int)b, __builtin_amdgcn_readlane((int)rch, c));
            if (rowok && t - lane < rl) {   // (unsigned: t >= lane) column j = t - lane + 1 is inside the matrix
                const int V = max(upH + go, upV + ge);
                Hz = max(Hcur + go, Hz + ge);
                const int h = max(diag + cell_score<KIND>(tab, qa, b), max(V, Hz));
                if (h > rmax) { rmax = h; rj = t - lane + 1; }
                Hcur = h; Vcur = V; diag = upH;
            }
            if (!last) {    // lane 63's cell of this step (column t - 62) goes to slot c of the outgoing registers
                outH = lane == c ? __builtin_amdgcn_readlane(Hcur, 63) : outH;
                outV = lane == c ? __builtin_amdgcn_readlane(Vcur, 63) : outV;
                if (c == 63u || t + 1 == T) {   // slot s holds column t - c + s - 62
                    const int jo = (int)(t - c + lane) - 62;
                    if (lane <= c && jo >= 1 && jo <= (int)rl) rowbuf[jo] = make_int2(outH, outV);
                }
            }
        }
        // the next band's loads follow this band's stores in the same wave
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) corner = __builtin_amdgcn_readlane(Hcur, (int)nb - 1);
        if (extend) {
            uint32_t lim = nb;
            if (xdrop) {   // rows in order: the running maximum includes the row itself; the first row that falls x_drop below it is the last one
                const int run = max(best, wave_incl_max(rowok ? rmax : NEG, lane));
                const unsigned long long stop = __ballot(rowok && rmax < run - xp.x_drop);
                if (stop) {
                    const uint32_t sl = (uint32_t)__builtin_ctzll(stop);
                    lim = sl + 1; rows = i0 + sl + 2; stopped = true;
                }
            }
            const int v = lane < lim ? rmax : NEG;
            const int m = wave_max_i(v);
            if (m > best) {   // ties: the smallest row, then (rj) the smallest column
                const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(lane < lim && v == m));
                best = m; bi = i0 + l + 1; bj = (uint32_t)__shfl((int)rj, (int)l, 64);
            }
        }
    }
    if (lane == 0) {
        ba::Exact o;
        if (extend) { o.score = best; o.query_idx = bi; o.reference_idx = bj; o.rows = rows; }
        else { o.score = corner; o.query_idx = ql; o.reference_idx = rl; o.rows = ql + 1; }
        *out = o;
    }
}

}  // namespace

template <int KIND>
__global__ void __launch_bounds__(64 * ba::EXACT_WAVES) k_exact(const ba::ExactParams xp) {
    __shared__ int8_t tab[1024];
    for (uint32_t k = threadIdx.x; k < 1024u; k += blockDim.x) tab[k] = k < xp.matrix_bytes ? xp.matrix[k] : (int8_t)0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    int2* rowbuf = (int2*)xp.rows + (uint64_t)(blockIdx.x * ba::EXACT_WAVES + w) * xp.row_stride;
    for (;;) {
        // (a convergence point: without it the compiler threads the "lane 0 writes the record" branch at the end of one pair into the
        // "lane 0 takes the next record" branch of the next, and the wave-wide operations below run with lane 0 apart from the others)
        __builtin_amdgcn_wave_barrier();
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(xp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= xp.n) break;
        const uint32_t d = xp.work[2 * k];
        ba::Exact* out = xp.out + xp.work[2 * k + 1];
        if (d == ba::EXACT_NO_PAIR) { if (lane == 0) *out = ba::Exact{}; continue; }
        exact_pair<KIND>(xp, tab, rowbuf, lane, d, out);
    }
}

// Extension batches: the score of every requested seed's ungapped columns (read from seed_pool, as the splice reads them); one thread per
// record.
__global__ void __launch_bounds__(256) k_exact_seed(const ba::ExtendParams ep, const uint32_t* __restrict__ which, uint32_t m, int32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t s = which[k];
    const uint32_t L = ep.seed_len[s];
    const uint8_t* qs = ep.seed_pool + ep.seed_q[s] + 1;
    const uint8_t* rs = ep.seed_pool + ep.seed_r[s] + 1;
    int sc = 0;
    for (uint32_t x = 0; x < L; x++) {
        const uint32_t a = qs[x], b = rs[x];
        if (ep.kind == ba::KIND_NUC) sc += ep.matrix[(a & 7u) * 16u + (b & 15u)];
        else if (ep.kind == ba::KIND_AA) sc += ep.matrix[min(a, 26u) * 32u + min(b, 31u)];
        else sc += a == b ? ep.matrix[0] : ep.matrix[1];
    }
    out[k] = sc;
}

extern "C" hipError_t ba_launch_exact(hipStream_t s, const ba::ExactParams* xp, uint32_t wgs) {
    if (!xp->n || !wgs) return hipSuccess;
    const dim3 g(wgs), b(64 * ba::EXACT_WAVES);
    if (xp->kind == ba::KIND_NUC) k_exact<ba::KIND_NUC><<<g, b, 0, s>>>(*xp);
    else if (xp->kind == ba::KIND_AA) k_exact<ba::KIND_AA><<<g, b, 0, s>>>(*xp);
    else k_exact<ba::KIND_BYTES><<<g, b, 0, s>>>(*xp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_exact_seed(hipStream_t s, const ba::ExtendParams* ep, const uint32_t* which, uint32_t m, int32_t* out) {
    if (!m) return hipSuccess;
    k_exact_seed<<<dim3((m + 255) / 256), dim3(256), 0, s>>>(*ep, which, m, out);
    return hipGetLastError();
}
