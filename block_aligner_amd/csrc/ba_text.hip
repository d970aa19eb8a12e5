// Alignment strings (ba_*_text, ba_host.cpp): the CIGAR, SAM MD:Z and minimap2 short cs:Z text of every traced alignment, rendered from the
// batch's CIGAR runs and sequences where the fill left them. k_text_len sizes every pair's text, k_text_offsets scans the sizes in the
// caller's order, k_text_write renders. No fill kernel is touched.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

constexpr uint32_t TEXT_WAVES = 4;   // waves per workgroup of k_text_len / k_text_write

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
__device__ __forceinline__ uint32_t lane_of(uint32_t x, uint32_t l) { return (uint32_t)__shfl((int)x, (int)l, 64); }

// decimal digits of v
__device__ __forceinline__ uint32_t ndig(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
__device__ __forceinline__ void put_num(char* p, uint32_t v, uint32_t nd) {
    for (uint32_t k = nd; k-- > 0;) { p[k] = (char)('0' + v % 10u); v /= 10u; }
}
__device__ __forceinline__ uint32_t upper(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32u : c; }
__device__ __forceinline__ uint32_t lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32u : c; }
__device__ __forceinline__ uint32_t complement(uint32_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
__device__ __forceinline__ char op_char(uint32_t op) { return op == 1u ? 'M' : op == 2u ? '=' : op == 3u ? 'X' : op == 4u ? 'I' : op == 5u ? 'D' : '?'; }

// one pair's two sequences as the letters of its image bytes: uppercase for NucMatrix, 'A' + code for AAMatrix; on the raw bytes of an
// extension batch, k_pack_images' rule (uppercase, the query reverse-complemented on the minus strand)
struct Letters {
    const uint8_t* q; const uint8_t* r; uint32_t ql; bool raw, minus, aa;
    __device__ __forceinline__ uint32_t qa(uint32_t i) const {
        if (!raw) return aa ? q[i] + (uint32_t)'A' : q[i];
        const uint32_t c = upper(q[minus ? ql - 1u - i : i]);
        return minus ? complement(c) : c;
    }
    __device__ __forceinline__ uint32_t ra(uint32_t j) const {
        if (!raw) return aa ? r[j] + (uint32_t)'A' : r[j];
        return upper(r[j]);
    }
};

// One wave per pair, pairs in the batch's device order, grid-stride; WRITE = false sizes the text (k_text_len), true renders it at
// offsets[caller position] (k_text_write). Both walk the same tokens, so the sizes are the rendered lengths; every store is also checked
// against the pair's end offset.
//
// The start cell comes first, from one sum over the runs (the end less what they consume). Then the runs are read forward, 64 at a time.
// CIGAR: lane k renders run k; a wave prefix sum of the token lengths places them. MD / cs: the chunk's "items" -- every cell of a
// match-type run, and every gap run as one item -- are spread over the lanes 64 at a time, in alignment order. Each match cell compares its
// two letters; a ballot gives the breaks (a mismatch, a D run, and in cs an I run too) and the equal cells. A break's token is the count of
// equal cells since the previous break -- popcounts of the masks, plus the wave-uniform count carried in from earlier items -- followed by
// its letters. Token offsets are a wave prefix sum; the letters of a gap run are written by the whole wave.
template <bool WRITE>
__device__ __forceinline__ void text_pairs(const ba::TextParams& tp, uint32_t (*sh)[64]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    // per wave, the chunk's runs: items up to and including run k; its first cell's i and j; the run itself
    uint32_t* incl = sh[0];
    uint32_t* ri = sh[1];
    uint32_t* rj = sh[2];
    uint32_t* rx = sh[3];
    const uint32_t fmt = tp.what & ba::TEXT_FORMAT;
    const bool clip = (tp.what & ba::TEXT_SOFT_CLIP) != 0, md = fmt == ba::TEXT_MD;
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull;   // the lanes before this one
    for (uint32_t d = blockIdx.x * TEXT_WAVES + w; d < tp.n; d += gridDim.x * TEXT_WAVES) {
        const uint32_t at_c = tp.out_pos ? tp.out_pos[d] : d;
        const uint32_t nr = (tp.status[d] & ba::STATS_FAILED) ? 0u : tp.nrun[d];
        const uint32_t* ops = tp.ops + (tp.run_end[d + 1] - nr);
        const uint32_t qe = tp.q_end[d], re = tp.r_end[d], ql = tp.q_len[d], rl = tp.r_len[d];
        uint32_t cq = 0, cr = 0;
        for (uint32_t k = lane; k < nr; k += 64u) {
            const uint32_t x = ops[k], op = x & 15u, len = x >> 4;
            const bool m = op >= 1u && op <= 3u;
            cq += (m || op == 4u) ? len : 0u;
            cr += (m || op == 5u) ? len : 0u;
        }
        cq = wave_sum(cq); cr = wave_sum(cr);
        // (runs that consume more than the end cell, or an end past the sequences, would read outside them: empty text. Never for the library's own runs.)
        const bool ok = nr > 0 && cq <= qe && cr <= re && (fmt == ba::TEXT_CIGAR ? qe <= ql : (qe <= ql && re <= rl));
        uint64_t pos = 0, lim = 0;
        char* const out = tp.text;
        if (WRITE) { pos = tp.offsets[at_c]; lim = tp.offsets[at_c + 1]; }
        const uint64_t base = pos;
        if (ok && fmt == ba::TEXT_CIGAR) {
            const uint32_t q0 = qe - cq, tail = ql - qe;
            if (clip && q0) {
                const uint32_t nd = ndig(q0);
                if (WRITE && lane == 0 && pos + nd + 1u <= lim) { put_num(out + pos, q0, nd); out[pos + nd] = 'S'; }
                pos += nd + 1u;
            }
            for (uint32_t lo = 0; lo < nr; lo += 64u) {
                const uint32_t cnt = min(nr - lo, 64u);
                const uint32_t x = lane < cnt ? ops[lo + lane] : 0u, len = x >> 4, nd = ndig(len);
                const uint32_t tl = lane < cnt ? nd + 1u : 0u;
                const uint32_t s = wave_incl_sum(tl, lane);
                const uint64_t at = pos + (s - tl);
                if (WRITE && tl && at + tl <= lim) { put_num(out + at, len, nd); out[at + nd] = op_char(x & 15u); }
                pos += lane_of(s, 63);
            }
            if (clip && tail) {
                const uint32_t nd = ndig(tail);
                if (WRITE && lane == 0 && pos + nd + 1u <= lim) { put_num(out + pos, tail, nd); out[pos + nd] = 'S'; }
                pos += nd + 1u;
            }
        } else if (ok) {
            Letters L;
            L.raw = tp.strand != nullptr; L.minus = L.raw && tp.strand[d]; L.aa = tp.kind == ba::KIND_AA; L.ql = ql;
            L.q = tp.seq + tp.q_off[d] + tp.skip; L.r = tp.seq + tp.r_off[d] + tp.skip;
            uint32_t ci = qe - cq, cj = re - cr;   // first cell of the chunk being read
            uint32_t carry = 0;                    // equal cells since the last break, before the current group of items
            for (uint32_t lo = 0; lo < nr; lo += 64u) {
                const uint32_t cnt = min(nr - lo, 64u);
                const uint32_t x = lane < cnt ? ops[lo + lane] : 0u, op = x & 15u, len = x >> 4;
                const bool m = op >= 1u && op <= 3u, gi = op == 4u, gd = op == 5u;
                const uint32_t uq = (m || gi) ? len : 0u, ur = (m || gd) ? len : 0u, ui = m ? len : ((gi || gd) ? 1u : 0u);
                const uint32_t sq = wave_incl_sum(uq, lane), sr = wave_incl_sum(ur, lane), si = wave_incl_sum(ui, lane);
                const uint32_t tq = lane_of(sq, 63), tr = lane_of(sr, 63), ti = lane_of(si, 63);
                incl[lane] = si; ri[lane] = ci + (sq - uq); rj[lane] = cj + (sr - ur); rx[lane] = x;
                wave_lds_fence();
                uint32_t k = 0, kend = incl[0];
                for (uint32_t t0 = 0; t0 < ti; t0 += 64u) {
                    const uint32_t t = t0 + lane;
                    const bool valid = t < ti;
                    if (valid && t >= kend) {
                        do k++; while (incl[k] <= t);   // (t < ti = incl[63]: ends inside the chunk)
                        kend = incl[k];
                    }
                    const uint32_t xk = rx[k], opk = xk & 15u, lenk = xk >> 4;
                    const bool mk = opk >= 1u && opk <= 3u;
                    uint32_t a = 0, b = 0;
                    if (valid && mk) {
                        const uint32_t off = t - (kend - lenk);
                        a = L.qa(ri[k] + off); b = L.ra(rj[k] + off);
                    }
                    const bool brk = valid && (mk ? a != b : (md ? opk == 5u : true));
                    const bool equal = valid && mk && a == b;
                    const uint64_t B = __ballot(brk), E = __ballot(equal);
                    // equal cells between the previous break (in this group, or before it: the carry) and this item
                    const uint64_t pb = B & below;
                    uint32_t nb;
                    if (pb) nb = (uint32_t)__popcll(E & below & ~((2ull << (63 - __builtin_clzll(pb))) - 1ull));
                    else nb = carry + (uint32_t)__popcll(E & below);
                    uint32_t nl = 0, tl = 0;   // the count's bytes, the token's bytes
                    if (brk) {
                        nl = md ? ndig(nb) : (nb ? 1u + ndig(nb) : 0u);
                        tl = nl + (mk ? (md ? 1u : 3u) : 1u + lenk);
                    }
                    const uint32_t s = wave_incl_sum(tl, lane);
                    if (WRITE) {
                        const uint64_t at = pos + (s - tl);
                        if (brk && at + tl <= lim) {
                            char* p = out + at;
                            if (md) put_num(p, nb, nl);
                            else if (nl) { p[0] = ':'; put_num(p + 1, nb, nl - 1u); }
                            p += nl;
                            if (mk && md) p[0] = (char)b;
                            else if (mk) { p[0] = '*'; p[1] = (char)lower(b); p[2] = (char)lower(a); }
                            else p[0] = md ? '^' : (opk == 4u ? '+' : '-');
                        }
                        // the letters of the group's gap runs, one run at a time, by the whole wave
                        for (uint64_t G = __ballot(brk && !mk); G; G &= G - 1ull) {
                            const uint32_t l = (uint32_t)__builtin_ctzll(G);
                            const uint32_t kk = lane_of(k, l), rel = lane_of(s - tl + nl + 1u, l);
                            const uint32_t xx = rx[kk], cntl = xx >> 4;
                            const bool ins = (xx & 15u) == 4u;
                            const uint32_t src = ins ? ri[kk] : rj[kk];
                            const uint64_t a0 = pos + rel;
                            if (a0 + cntl <= lim)
                                for (uint32_t u = lane; u < cntl; u += 64u) {
                                    const uint32_t c = ins ? L.qa(src + u) : L.ra(src + u);
                                    out[a0 + u] = (char)(md ? c : lower(c));
                                }
                        }
                    }
                    pos += lane_of(s, 63);
                    if (B) carry = (uint32_t)__popcll(E & ~((2ull << (63 - __builtin_clzll(B))) - 1ull));   // (last break in lane 63: 2 << 63 = 0, none)
                    else carry += (uint32_t)__popcll(E);
                }
                wave_lds_fence();   // (the next chunk overwrites the table)
                ci += tq; cj += tr;
            }
            // the count after the last break
            const uint32_t nl = md ? ndig(carry) : (carry ? 1u + ndig(carry) : 0u);
            if (WRITE && lane == 0 && nl && pos + nl <= lim) {
                if (md) put_num(out + pos, carry, nl);
                else { out[pos] = ':'; put_num(out + pos + 1, carry, nl - 1u); }
            }
            pos += nl;
        }
        if (!WRITE && lane == 0) tp.len[at_c] = (uint32_t)(pos - base);
    }
}

}  // namespace

__global__ void __launch_bounds__(256) k_text_len(const ba::TextParams tp) {
    __shared__ uint32_t sh[TEXT_WAVES][4][64];
    text_pairs<false>(tp, sh[threadIdx.x >> 6]);
}
__global__ void __launch_bounds__(256) k_text_write(const ba::TextParams tp) {
    __shared__ uint32_t sh[TEXT_WAVES][4][64];
    text_pairs<true>(tp, sh[threadIdx.x >> 6]);
}

// offsets[p] = sum of len over the pairs before p (caller order), offsets[n] = the total. One workgroup: per-thread chunk sums, a scan over the
// 1024 partial sums, a second pass over the chunks.
__global__ void __launch_bounds__(1024) k_text_offsets(const uint32_t* __restrict__ len, uint64_t* __restrict__ offsets, uint32_t n) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (uint32_t p = lo; p < hi; p++) sum += len[p];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive scan
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long at = part[t] - sum;
    for (uint32_t p = lo; p < hi; p++) { offsets[p] = at; at += len[p]; }
    if (t == 1023) offsets[n] = part[1023];
}

// the sizes and their offsets (k_text_len, k_text_offsets)
extern "C" hipError_t ba_launch_text_len(hipStream_t s, const ba::TextParams* tp) {
    if (!tp->n) return hipSuccess;
    const uint32_t wgs = (tp->n + TEXT_WAVES - 1) / TEXT_WAVES;
    k_text_len<<<dim3(wgs < 2048u ? wgs : 2048u), dim3(64 * TEXT_WAVES), 0, s>>>(*tp);
    k_text_offsets<<<dim3(1), dim3(1024), 0, s>>>(tp->len, tp->offsets, tp->n);
    return hipGetLastError();
}
// the scan on its own (the exact paths' run offsets): offsets[0 .. n] of len[0 .. n)
extern "C" hipError_t ba_launch_offsets(hipStream_t s, const uint32_t* len, uint64_t* offsets, uint32_t n) {
    k_text_offsets<<<dim3(1), dim3(1024), 0, s>>>(len, offsets, n);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_text_write(hipStream_t s, const ba::TextParams* tp) {
    if (!tp->n) return hipSuccess;
    const uint32_t wgs = (tp->n + TEXT_WAVES - 1) / TEXT_WAVES;
    k_text_write<<<dim3(wgs < 2048u ? wgs : 2048u), dim3(64 * TEXT_WAVES), 0, s>>>(*tp);
    return hipGetLastError();
}
