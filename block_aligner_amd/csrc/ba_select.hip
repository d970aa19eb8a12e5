// Read-level selection (ba_select_*, ba_host.cpp): from candidates in any order -- chains before alignment, alignments after it -- to the
// marks of a mapper's records: which of a read's candidates is primary, which are supplementary or secondary, which are dropped, and the
// mapping quality of the heads. The rule is stated in INTEGRATION.md, "Selecting a read's alignments"; everything is integer arithmetic, so
// the kernels equal the model of tests/select_ref.py bit for bit.
//
// k_select_group: the grouping, in two passes around a scan of the counts. Pass 0, a thread per candidate: eligibility and the span in the
// read's own frame, one atomicAdd on the read's count; a candidate that is not eligible gets its final outputs here. Pass 1: an atomic
// cursor per read places the sort key (~biased score) << 32 | c in the read's slice. The order inside a slice is arbitrary; the key is
// total, so the sort removes it.
// k_select_mark: the marking. One wave (a workgroup of its own) per read at a time, persistent, the reads with the most candidates first
// through a work counter. The read's keys are sorted in LDS by the bitonic network of ba_seed_device.hpp. The wave loads 64 candidates at
// once, one per lane, and takes them one after the other in rank order (v_readlane broadcasts the candidate). The heads' (a, b, rank, sub)
// sit in LDS in rank order; 64 of them are tested per step, and the lowest set bit of the ballot is the first head that passes. The number
// of heads, of secondaries and of kept candidates are the wave's scalars. The mapping quality is computed when the sweep is done, a head
// per lane. The sorted keys go back to the read's slice for the emit.
// k_select_emit: one wave per read writes the read's kept candidates in rank order, 64 ranks per step by a ballot and a prefix count.
#include <hip/hip_runtime.h>

#include "ba_launch.h"
#include "ba_seed_device.hpp"

namespace {

using ba::seed::bcast;
using ba::seed::wave_sync;
constexpr uint32_t NONE = ba::SELECT_NONE;
constexpr uint32_t BIAS = 0x80000000u;   // int32 -> uint32, order kept
constexpr uint32_t MAXC = ba::SELECT_MAX_PER_READ;

__device__ __forceinline__ uint64_t key_of(int32_t score, uint32_t c) { return (uint64_t)(~((uint32_t)score ^ BIAS)) << 32 | c; }
__device__ __forceinline__ int32_t score_of(uint64_t key) { return (int32_t)(~(uint32_t)(key >> 32) ^ BIAS); }

}  // namespace

__global__ void __launch_bounds__(256) k_select_group(const ba::SelectParams sp, const int scatter) {
    for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < sp.n; c += gridDim.x * 256u) {
        const uint32_t r = sp.read[c];
        if (scatter) {
            if (sp.b[c] > sp.a[c]) sp.keys[sp.first[r] + atomicAdd(sp.cursor + r, 1u)] = key_of(sp.score[c], c);
            continue;
        }
        const uint32_t qs = sp.q_start[c], qe = sp.q_end[c], ql = sp.q_len[c];
        const bool minus = sp.strand && sp.strand[c];
        bool ok = r < sp.n_reads && qs <= qe && qe <= ql && sp.score[c] >= sp.min_score;   // (the first three: the host's checks, held again)
        if (sp.exclude && sp.exclude[c]) ok = false;
        if (sp.status && (sp.status[c] & sp.failed)) ok = false;
        uint32_t a = minus ? ql - qe : qs, b = minus ? ql - qs : qe;
        if (!ok || b <= a) {
            a = b = 0;
            sp.cls[c] = ba::SEL_EXCLUDED; sp.mapq[c] = 0; sp.parent[c] = NONE; sp.rank[c] = NONE; sp.sub_score[c] = 0;
        } else atomicAdd(sp.count + r, 1u);
        sp.a[c] = a; sp.b[c] = b;
    }
}

__global__ void __launch_bounds__(64) k_select_mark(const ba::SelectParams sp) {
    __shared__ uint64_t keys[MAXC];
    __shared__ uint32_t ha[MAXC], hb[MAXC], hrank[MAXC];
    __shared__ int32_t hsub[MAXC];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        __builtin_amdgcn_wave_barrier();   // (a convergence point, as in k_chaining_fill)
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(sp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= sp.n_reads) break;
        const uint32_t r = sp.order[k];
        const uint64_t f0 = sp.first[r];
        const uint64_t have = sp.first[r + 1] - f0;
        const uint32_t cnt = have < MAXC ? (uint32_t)have : MAXC;   // (the host admits no read with more)
        for (uint32_t i = lane; i < cnt; i += 64u) keys[i] = sp.keys[f0 + i];
        __syncthreads();   // (the workgroup is this wave)
        ba::seed::sort_network<64>(keys, cnt);
        uint32_t nh = 0, nsec = 0, kept = 0;
        for (uint32_t base = 0; base < cnt; base += 64u) {
            const uint32_t il = base + lane;
            const bool in = il < cnt;
            const uint64_t key = in ? keys[il] : 0ull;
            const uint32_t c = (uint32_t)key;
            const uint32_t sc = (uint32_t)score_of(key);
            uint32_t la = 0, lb = 0;
            if (in) { la = sp.a[c]; lb = sp.b[c]; sp.keys[f0 + il] = key; }
            uint32_t my_cls = ba::SEL_EXCLUDED, my_parent = NONE;
            const uint32_t steps = cnt - base < 64u ? cnt - base : 64u;
            for (uint32_t t = 0; t < steps; t++) {
                const uint32_t ai = bcast(la, t), bi = bcast(lb, t), ci = bcast(c, t), span = bi - ai;
                const int32_t si = (int32_t)bcast(sc, t);
                uint32_t found = NONE;
                for (uint32_t h0 = 0; h0 < nh; h0 += 64u) {
                    const uint32_t hl = h0 + lane;
                    bool pass = false;
                    if (hl < nh) {
                        const uint32_t ah = ha[hl], bh = hb[hl];
                        const uint32_t lo = ai > ah ? ai : ah, hi = bi < bh ? bi : bh, sh = bh - ah;
                        pass = hi > lo && 1000ull * (hi - lo) >= (uint64_t)sp.mask_permille * (span < sh ? span : sh);
                    }
                    const uint64_t m = __ballot(pass);
                    if (m) { found = h0 + (uint32_t)__builtin_ctzll(m); break; }
                }
                uint32_t cls, par;
                if (found != NONE) {
                    const uint64_t hkey = keys[hrank[found]];
                    if (lane == 0 && hsub[found] < si) hsub[found] = si;
                    const bool sec = 1000ll * si >= (int64_t)sp.sec_permille * score_of(hkey) && nsec < sp.max_secondary;
                    cls = sec ? ba::SEL_SECONDARY : ba::SEL_DROPPED; par = (uint32_t)hkey;
                    nsec += sec ? 1u : 0u;
                } else {
                    if (lane == 0) { ha[nh] = ai; hb[nh] = bi; hrank[nh] = base + t; hsub[nh] = 0; }
                    cls = base + t == 0u ? ba::SEL_PRIMARY : ba::SEL_SUPPLEMENTARY; par = ci;
                    nh++;
                }
                kept += cls <= ba::SEL_SECONDARY ? 1u : 0u;
                if (lane == t) { my_cls = cls; my_parent = par; }
                wave_sync();
            }
            if (in) {
                sp.cls[c] = (uint8_t)my_cls; sp.parent[c] = my_parent; sp.rank[c] = il;
                if (my_cls >= ba::SEL_SECONDARY) { sp.mapq[c] = 0; sp.sub_score[c] = 0; }   // (a head's: below)
            }
        }
        for (uint32_t h = lane; h < nh; h += 64u) {
            const uint64_t hkey = keys[hrank[h]];
            const uint32_t c = (uint32_t)hkey;
            const int32_t s1 = score_of(hkey), s2 = hsub[h];
            uint32_t u = sp.full_support;
            if (sp.support && sp.support[c] < u) u = sp.support[c];
            sp.mapq[c] = (uint8_t)(((uint64_t)sp.mapq_max * (uint32_t)(s1 - s2) * u) / ((uint64_t)(uint32_t)s1 * sp.full_support));
            sp.sub_score[c] = s2;
        }
        if (lane == 0) sp.n_kept[r] = kept;
        __syncthreads();   // the next read's keys and heads take the same LDS
    }
}

constexpr uint32_t SELECT_WAVES = 4;   // waves per workgroup of k_select_emit: one read per wave at a time

__global__ void __launch_bounds__(64 * SELECT_WAVES) k_select_emit(const ba::SelectParams sp) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x * SELECT_WAVES + w; r < sp.n_reads; r += gridDim.x * SELECT_WAVES) {
        const uint64_t f0 = sp.first[r];
        const uint32_t cnt = (uint32_t)(sp.first[r + 1] - f0);
        uint64_t at = sp.kept_first[r];
        for (uint32_t base = 0; base < cnt; base += 64u) {
            const bool in = base + lane < cnt;
            const uint32_t c = in ? (uint32_t)sp.keys[f0 + base + lane] : 0u;
            const bool keep = in && sp.cls[c] <= ba::SEL_SECONDARY;
            const uint64_t m = __ballot(keep);
            if (keep) sp.kept[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = c;
            at += (uint32_t)__popcll(m);
        }
    }
}

extern "C" hipError_t ba_launch_select_group(hipStream_t s, const ba::SelectParams* sp, int scatter) {
    const uint32_t wgs = (sp->n + 255u) / 256u;
    k_select_group<<<dim3(wgs < 2048u ? wgs : 2048u), dim3(256), 0, s>>>(*sp, scatter);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_select_mark(hipStream_t s, const ba::SelectParams* sp) {
    k_select_mark<<<dim3(sp->n_reads < 2048u ? sp->n_reads : 2048u), dim3(64), 0, s>>>(*sp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_select_emit(hipStream_t s, const ba::SelectParams* sp) {
    const uint32_t wgs = (sp->n_reads + SELECT_WAVES - 1u) / SELECT_WAVES;
    k_select_emit<<<dim3(wgs < 4096u ? wgs : 4096u), dim3(64 * SELECT_WAVES), 0, s>>>(*sp);
    return hipGetLastError();
}
