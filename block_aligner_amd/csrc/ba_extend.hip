// Seed-and-extend batches (ba_extend_batch_*, ba_host.cpp): the image packer for the sides of the seeds and the splice behind the fill.
// The fill itself is an ordinary batch over every non-empty side; its kernels are untouched.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

__device__ inline uint32_t complement(uint32_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

// the fill's score of query byte a against reference byte b (converted bytes)
__device__ inline int pair_score(int kind, const int8_t* __restrict__ m, uint32_t a, uint32_t b) {
    if (kind == ba::KIND_NUC) return m[(a & 7) * 16 + (b & 15)];
    if (kind == ba::KIND_AA) return m[a * 32 + b];
    return a == b ? m[0] : m[1];
}

}  // namespace

// PaddedBytes images ([NULL] + convert(bytes) + NULL x pad) of slices of the caller's raw bytes, as k_pack_sequences builds them (ba_kernels.hip),
// each with its own IMG_* flags: a forward slice, a reversed prefix, a (reverse) complemented piece. One workgroup per image, blockIdx.x = 2 x pair +
// (0 query, 1 reference); flags[blockIdx.x]. A byte the reference would assert on is reported through *err (lowest pair wins): pair << 8 | byte.
__global__ void __launch_bounds__(256) k_pack_images(int kind, const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_q,
                                                     const uint64_t* __restrict__ raw_r, const uint8_t* __restrict__ flags,
                                                     const uint64_t* __restrict__ q_off, const uint32_t* __restrict__ q_len,
                                                     const uint64_t* __restrict__ r_off, const uint32_t* __restrict__ r_len,
                                                     uint8_t* __restrict__ image, uint32_t pad, unsigned long long* err) {
    const uint32_t p = blockIdx.x >> 1;
    const bool ref = blockIdx.x & 1;
    const uint8_t* src = raw + (ref ? raw_r[p] : raw_q[p]);
    const uint32_t len = ref ? r_len[p] : q_len[p];
    const uint32_t f = flags[blockIdx.x];
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
                const uint32_t byte = src[(f & ba::IMG_REVERSE) ? len - pos : pos - 1];
                c = byte;
                if (kind != ba::KIND_BYTES) {
                    if (c >= 'a' && c <= 'z') c -= 32;
                    if (f & ba::IMG_COMPLEMENT) c = complement(c);
                    const bool ok = kind == ba::KIND_AA ? (c >= 'A' && c <= 'A' + 26) : (c >= 'A' && c <= 'Z');
                    if (!ok) { atomicMin(err, ((unsigned long long)p << 8) | byte); c = null_b; }
                    else if (kind == ba::KIND_AA) c -= 'A';
                }
            }
            wd |= c << (8 * b);
        }
        dst[k] = wd;
    }
}
extern "C" hipError_t ba_launch_pack_images(hipStream_t s, int kind, const uint8_t* raw, const uint64_t* raw_q, const uint64_t* raw_r, const uint8_t* flags,
                                            const uint64_t* q_off, const uint32_t* q_len, const uint64_t* r_off, const uint32_t* r_len,
                                            uint8_t* image, uint32_t pad, uint32_t n, unsigned long long* err) {
    k_pack_images<<<dim3(2 * n), dim3(256), 0, s>>>(kind, raw, raw_q, raw_r, flags, q_off, q_len, r_off, r_len, image, pad, err);
    return hipGetLastError();
}

// Splice, pass 1: one thread per seed. Seed score (and, with TRACE, the seed's runs), both sides' results read from the inner batch, the
// combined result; with TRACE the number of runs after the joins merge: the left side's first run (the one next to the seed) with the seed's
// first run, the seed's last run with the right side's first run, where their ops are the same.
__global__ void __launch_bounds__(256) k_extend_results(const ba::ExtendParams ep) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ep.n) return;
    const bool trace = ep.flags & ba::F_TRACE, eq = ep.flags & ba::F_CIGAR_EQ;
    const uint32_t L = ep.seed_len[s];
    const uint8_t* qs = ep.seed_pool + ep.seed_q[s] + 1;
    const uint8_t* rs = ep.seed_pool + ep.seed_r[s] + 1;
    int sc = 0;
    uint32_t nrun = 0, first_op = 0, last_op = 0;
    for (uint32_t k = 0; k < L; k++) {
        const uint32_t a = qs[k], b = rs[k];
        sc += pair_score(ep.kind, ep.matrix, a, b);
        const uint32_t op = eq ? (a == b ? 2u : 3u) : 1u;
        if (op != last_op) { nrun++; if (!first_op) first_op = op; last_op = op; }
    }
    const uint32_t dl = ep.side[2 * s], dr = ep.side[2 * s + 1];
    const bool hl = dl != ba::EXT_NO_SIDE, hr = dr != ba::EXT_NO_SIDE;
    const int ls = hl ? ep.in_score[dl] : 0, rsc = hr ? ep.in_score[dr] : 0;
    ep.score[s] = ls + sc + rsc; ep.left_score[s] = ls; ep.right_score[s] = rsc;
    ep.q_start[s] = ep.q_seed[s] - (hl ? ep.in_qidx[dl] : 0u);
    ep.r_start[s] = ep.r_seed[s] - (hl ? ep.in_ridx[dl] : 0u);
    ep.q_end[s] = ep.q_seed[s] + L + (hr ? ep.in_qidx[dr] : 0u);
    ep.r_end[s] = ep.r_seed[s] + L + (hr ? ep.in_ridx[dr] : 0u);
    ep.cells[s] = (hl ? ep.in_cells[dl] : 0ull) + (hr ? ep.in_cells[dr] : 0ull);
    ep.status[s] = (hl ? ep.in_status[dl] : 0u) | (hr ? ep.in_status[dr] : 0u);
    if (!trace) return;
    const uint32_t nl = hl ? ep.in_cig_len[dl] : 0u, nr = hr ? ep.in_cig_len[dr] : 0u;
    const uint32_t ml = nl && (ep.in_cig_ops[ep.in_cig_off[dl + 1] - nl] & 15u) == first_op;
    const uint32_t mr = nr && (ep.in_cig_ops[ep.in_cig_off[dr + 1] - nr] & 15u) == last_op;
    ep.cigar_len[s] = nl + nrun + nr - ml - mr;
    ep.join[s] = nrun << 2 | mr << 1 | ml;
}

// Splice, pass 2: out_off[s] = sum of cigar_len over the seeds before s, out_off[n] = the total. One workgroup: per-thread chunk sums, a scan over
// the 1024 partial sums, a second pass (k_cigar_offsets, ba_kernels.hip, in the caller's order).
__global__ void __launch_bounds__(1024) k_extend_offsets(const uint32_t* __restrict__ cigar_len, uint64_t* __restrict__ out_off, uint32_t n) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (uint32_t p = lo; p < hi; p++) sum += cigar_len[p];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive scan
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long at = part[t] - sum;
    for (uint32_t p = lo; p < hi; p++) { out_off[p] = at; at += cigar_len[p]; }
    if (t == 1023) out_off[n] = part[1023];
}

// Splice, pass 3: the runs of seed s at out_off[s] -- the left side's runs in reverse order, the seed's runs, the right side's runs, merged at the
// joins as pass 1 decided. One workgroup per seed at a time; the sides' runs are copied by all threads, the seed's runs written by thread 0.
__global__ void __launch_bounds__(256) k_extend_gather(const ba::ExtendParams ep) {
    const bool eq = ep.flags & ba::F_CIGAR_EQ;
    for (uint32_t s = blockIdx.x; s < ep.n; s += gridDim.x) {
        const uint64_t o = ep.out_off[s];
        const uint32_t dl = ep.side[2 * s], dr = ep.side[2 * s + 1];
        const uint32_t nl = dl != ba::EXT_NO_SIDE ? ep.in_cig_len[dl] : 0u, nr = dr != ba::EXT_NO_SIDE ? ep.in_cig_len[dr] : 0u;
        const uint64_t srcl = nl ? ep.in_cig_off[dl + 1] - nl : 0, srcr = nr ? ep.in_cig_off[dr + 1] - nr : 0;
        const uint32_t join = ep.join[s], ml = join & 1u, mr = (join >> 1) & 1u, nrun = join >> 2;
        const uint32_t a = nl - ml;   // left runs written as they are (all but the one merged into the seed's first run)
        for (uint32_t k = threadIdx.x; k < a; k += blockDim.x) ep.runs[o + k] = ep.in_cig_ops[srcl + nl - 1 - k];
        const uint64_t c = o + a + nrun;
        for (uint32_t k = threadIdx.x; k < nr - mr; k += blockDim.x) ep.runs[c + k] = ep.in_cig_ops[srcr + mr + k];
        if (threadIdx.x == 0) {
            const uint32_t L = ep.seed_len[s];
            const uint8_t* qs = ep.seed_pool + ep.seed_q[s] + 1;
            const uint8_t* rs = ep.seed_pool + ep.seed_r[s] + 1;
            uint32_t op = 0, len = ml ? ep.in_cig_ops[srcl] >> 4 : 0u;   // the run being built; its length starts with the merged left run's
            uint64_t at = o + a;
            for (uint32_t k = 0; k < L; k++) {
                const uint32_t x = eq ? (qs[k] == rs[k] ? 2u : 3u) : 1u;
                if (x != op && op) { ep.runs[at++] = len << 4 | op; len = 0; }
                op = x; len++;
            }
            if (mr) len += ep.in_cig_ops[srcr] >> 4;
            ep.runs[at] = len << 4 | op;
        }
    }
}

extern "C" hipError_t ba_launch_extend_results(hipStream_t s, const ba::ExtendParams* ep) {
    k_extend_results<<<dim3((ep->n + 255) / 256), dim3(256), 0, s>>>(*ep);
    if (ep->flags & ba::F_TRACE) k_extend_offsets<<<dim3(1), dim3(1024), 0, s>>>(ep->cigar_len, ep->out_off, ep->n);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_extend_gather(hipStream_t s, const ba::ExtendParams* ep) {
    const unsigned grid = ep->n < 4096 ? ep->n : 4096;
    k_extend_gather<<<dim3(grid), dim3(256), 0, s>>>(*ep);
    return hipGetLastError();
}
