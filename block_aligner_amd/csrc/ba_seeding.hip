// Minimizer seeding (ba_seeding_*, ba_host.cpp): from the bytes of a problem -- one read against one reference stretch on one strand -- to its
// raw hits, sorted by (reference position, query position): what ba_chaining_create takes. The rule is stated in INTEGRATION.md, "Seeding";
// everything is integer arithmetic, so the kernels equal the model of tests/seeding_ref.py bit for bit.
//
// k_seeding_sketch<EMIT>: the (w, k)-minimizer sketch of every sequence, as a count pass and an emit pass with a scan of the counts between
// them. One wave per sequence at a time, persistent, the sequences longest first through a work counter. A chunk is 64 consecutive windows:
// the wave stages the chunk's bytes and a halo of k + w - 2 more in LDS as two-bit codes (4: not ACGT; a minus-strand query is read from its
// end and complemented), computes code and order key (h << 32 | pos, all ones for an invalid k-mer) of the 63 + w k-mers under those windows,
// one or two per lane, and every lane takes the minimum of its window's w keys. A window's minimizer is selected when it differs from the
// window's before it -- the minimizers of consecutive windows never go back --, and the selected ones are compacted by a ballot and a running
// count. A query's entries are also written as sort keys, code << 32 | pos.
// k_seeding_sort: one workgroup per problem sorts the query's keys with a normalized bitonic network: every compare-exchange is ascending,
// so an entry past the end would never move, and a pair whose partner lies past the end is skipped: no padding. Up to 8192 entries in LDS,
// more than that in the problem's own slice of global memory, the same network between workgroup barriers.
// k_seeding_match<EMIT>: one wave per problem, 64 reference entries per step, again a count pass, a scan and an emit pass. Every lane
// searches the lower and the upper bound of its code among the query's sorted keys; a count above max_occ becomes 0; a prefix sum over the
// wave and a running base give the place of the entry's hits.
#include <hip/hip_runtime.h>

#include "ba_launch.h"

namespace {

constexpr uint64_t NO_KEY = ~0ull;
constexpr uint32_t SKETCH_WAVES = 4, MATCH_WAVES = 4, SORT_THREADS = 1024;
constexpr uint32_t CHUNK_KEYS = 128, CHUNK_BYTES = 192;   // 64 windows: at most 63 + 64 k-mers over at most 63 + 64 + 15 bytes

struct SketchLds {   // one wave's
    uint64_t key[CHUNK_KEYS];
    uint32_t code[CHUNK_KEYS];
    uint8_t two[CHUNK_BYTES];
};

// lanes of one wave hand data to one another through LDS: program order is enough for the hardware, the compiler must keep it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t bcast(uint32_t x, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)lane); }
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= (uint32_t)d ? o : 0u;
    }
    return x;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64);
        x += (uint64_t)hi << 32 | lo;
    }
    return x;
}
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= 0x9e3779b9u;
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
// A, C, G, T in either case -> 0 .. 3, any other byte -> 4; rc: the complement. (Clearing bit 5 maps no byte but a and A onto A.)
__device__ __forceinline__ uint32_t two_bits(uint8_t c, bool rc) {
    c &= 0xdfu;
    const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    return rc && v < 4u ? 3u - v : v;
}
// the first index in a[0 .. n) whose key is not below x
__device__ __forceinline__ uint32_t lower_bound(const uint64_t* a, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// one compare-exchange of the sort: ascending, and skipped when the partner lies past the end
__device__ __forceinline__ void exchange(uint64_t* a, uint32_t i, uint32_t l, uint32_t n) {
    if (l < n) {
        const uint64_t x = a[i], y = a[l];
        if (x > y) { a[i] = y; a[l] = x; }
    }
}
// The normalized bitonic network over a[0 .. n), in LDS or in global memory, by all threads of the workgroup. Blocks of 2, 4, 8, ...: first
// every entry against its mirror image in the block, then halves of halves at distance j.
__device__ __forceinline__ void sort_network(uint64_t* a, uint32_t n) {
    uint32_t lg = 1;
    while ((1ull << lg) < n) lg++;
    const uint32_t pairs = 1u << (lg - 1u);
    for (uint32_t b = 1; b <= lg; b++) {   // blocks of 1 << b entries
        for (uint32_t t = threadIdx.x; t < pairs; t += SORT_THREADS) {
            const uint32_t i = (t >> (b - 1u)) << b | (t & ((1u << (b - 1u)) - 1u));
            exchange(a, i, i ^ ((1u << b) - 1u), n);
        }
        __syncthreads();
        for (uint32_t lj = b - 1u; lj-- > 0u;) {   // distance 1 << lj
            for (uint32_t t = threadIdx.x; t < pairs; t += SORT_THREADS) {
                const uint32_t i = (t >> lj) << (lj + 1u) | (t & ((1u << lj) - 1u));
                exchange(a, i, i + (1u << lj), n);
            }
            __syncthreads();
        }
    }
}

}  // namespace

template <bool EMIT> __global__ void __launch_bounds__(64 * SKETCH_WAVES) k_seeding_sketch(const ba::SeedingParams sp) {
    __shared__ SketchLds lds[SKETCH_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    SketchLds& L = lds[threadIdx.x >> 6];
    const uint32_t k = sp.k, w = sp.w, n_seq = 2u * sp.n;
    const uint32_t need_keys = 63u + w, need_bytes = need_keys + k - 1u;
    for (;;) {
        __builtin_amdgcn_wave_barrier();   // (a convergence point, as in k_chaining_fill)
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(sp.counter, 1u);
        __builtin_amdgcn_wave_barrier();
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= n_seq) break;
        const uint32_t s = sp.seq_order[t], len = sp.seq_len[s];
        const uint8_t* seq = sp.pool + sp.seq_off[s];
        const bool rc = sp.seq_rc[s] != 0;
        const uint32_t nk = len >= k ? len - k + 1u : 0u;                  // k-mers
        const uint32_t nw = nk == 0u ? 0u : nk > w ? nk - w + 1u : 1u;     // windows
        const uint64_t out0 = EMIT ? sp.seed_first[s] : 0ull;
        uint32_t count = 0;
        uint64_t prev = NO_KEY;   // the minimizer of the window before the chunk
        for (uint32_t s0 = 0; s0 < nw; s0 += 64u) {
            for (uint32_t b = lane; b < need_bytes; b += 64u) {
                const uint32_t i = s0 + b;
                uint32_t v = 4;
                if (i < len) v = two_bits(seq[rc ? len - 1u - i : i], rc);
                L.two[b] = (uint8_t)v;
            }
            wave_sync();
            for (uint32_t j = lane; j < need_keys; j += 64u) {
                const uint32_t pos = s0 + j;
                uint32_t code = 0, bad = 0;
                for (uint32_t x = 0; x < k; x++) {
                    const uint32_t v = L.two[j + x];
                    bad |= v;
                    code = code << 2 | (v & 3u);
                }
                L.key[j] = pos < nk && !(bad & 4u) ? (uint64_t)hash32(code) << 32 | pos : NO_KEY;
                L.code[j] = code;
            }
            wave_sync();
            uint64_t m = NO_KEY;   // (a window past the last one selects nothing)
            if (s0 + lane < nw)
                for (uint32_t x = 0; x < w; x++) {
                    const uint64_t c = L.key[lane + x];
                    m = c < m ? c : m;
                }
            const uint32_t bl = (uint32_t)__shfl_up((int)(uint32_t)m, 1, 64), bh = (uint32_t)__shfl_up((int)(uint32_t)(m >> 32), 1, 64);
            const uint64_t before = lane ? (uint64_t)bh << 32 | bl : prev;
            const bool take = m != NO_KEY && m != before;
            const uint64_t ballot = __ballot(take);
            if (EMIT && take) {
                const uint32_t pos = (uint32_t)m, code = L.code[pos - s0];
                const uint64_t at = out0 + count + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
                sp.seed_pos[at] = pos; sp.seed_code[at] = code;
                if (s < sp.n) sp.q_key[at] = (uint64_t)code << 32 | pos;   // (the queries' entries come first: the same index)
            }
            count += (uint32_t)__popcll(ballot);
            prev = (uint64_t)bcast((uint32_t)(m >> 32), 63) << 32 | bcast((uint32_t)m, 63);
            wave_sync();   // the next chunk overwrites what this one read
        }
        if (!EMIT && lane == 0) sp.seed_cnt[s] = count;
    }
}

__global__ void __launch_bounds__(SORT_THREADS) k_seeding_sort(const ba::SeedingParams sp) {
    __shared__ uint64_t keys[ba::SEEDING_SORT_LDS];
    for (uint32_t t = blockIdx.x; t < sp.n; t += gridDim.x) {
        const uint32_t p = sp.sort_order[t];
        const uint64_t a0 = sp.seed_first[p];
        const uint32_t cnt = (uint32_t)(sp.seed_first[p + 1] - a0);
        uint64_t* g = sp.q_key + a0;
        if (cnt < 2u) continue;
        if (cnt <= ba::SEEDING_SORT_LDS) {
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) keys[i] = g[i];
            __syncthreads();
            sort_network(keys, cnt);
            for (uint32_t i = threadIdx.x; i < cnt; i += SORT_THREADS) g[i] = keys[i];
            __syncthreads();   // the next problem overwrites the keys
        } else {
            sort_network(g, cnt);   // (__syncthreads orders the workgroup's global accesses as well)
        }
    }
}

template <bool EMIT> __global__ void __launch_bounds__(64 * MATCH_WAVES) k_seeding_match(const ba::SeedingParams sp) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x * MATCH_WAVES + wv; t < sp.n; t += gridDim.x * MATCH_WAVES) {
        const uint32_t p = sp.match_order[t];
        const uint64_t q0 = sp.seed_first[p], r0 = sp.seed_first[sp.n + p];
        const uint32_t qc = (uint32_t)(sp.seed_first[p + 1] - q0), rcnt = (uint32_t)(sp.seed_first[sp.n + p + 1] - r0);
        const uint64_t* qk = sp.q_key + q0;
        const uint64_t h0 = EMIT ? sp.hit_first[p] : 0ull;
        uint64_t total = 0;   // the lane's own hits (the count pass)
        uint32_t run = 0;     // the hits of the steps before (the emit pass: at most 2^28 in all)
        for (uint32_t base = 0; base < rcnt; base += 64u) {
            const uint32_t e = base + lane;
            uint32_t m = 0, lo = 0;
            if (e < rcnt && qc) {
                const uint64_t code = sp.seed_code[r0 + e];
                lo = lower_bound(qk, qc, code << 32);
                if (lo < qc && qk[lo] >> 32 == code) {   // (most codes of a reference are not in the query: no second search for them)
                    // (the end of the code's run: no position is 0xffffffff; code + 1 would leave 64 bits for the all-T 16-mer)
                    m = 1u + lower_bound(qk + lo + 1u, qc - lo - 1u, code << 32 | 0xffffffffull);
                    if (m > sp.max_occ) m = 0;
                }
            }
            if (EMIT) {
                const uint32_t incl = wave_incl_sum(m, lane);
                if (m) {
                    const uint64_t at = h0 + run + (incl - m);
                    const uint32_t rpos = sp.seed_pos[r0 + e];
                    for (uint32_t i = 0; i < m; i++) { sp.q_hit[at + i] = (uint32_t)qk[lo + i]; sp.r_hit[at + i] = rpos; sp.hit_len[at + i] = sp.k; }
                }
                run += bcast(incl, 63);
            } else {
                total += m;
            }
        }
        if (!EMIT) {
            total = wave_sum64(total);
            if (lane == 0) sp.hit_cnt[p] = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
        }
    }
}

// The sketch's count pass (emit 0: seed_cnt) or emit pass (seed_pos, seed_code, q_key at seed_first); the work counter is zeroed by the host.
extern "C" hipError_t ba_launch_seeding_sketch(hipStream_t s, const ba::SeedingParams* sp, int emit) {
    const uint32_t wgs = (2u * sp->n + SKETCH_WAVES - 1u) / SKETCH_WAVES;
    const dim3 grid(wgs < 2048u ? wgs : 2048u), block(64 * SKETCH_WAVES);
    if (emit) k_seeding_sketch<true><<<grid, block, 0, s>>>(*sp);
    else k_seeding_sketch<false><<<grid, block, 0, s>>>(*sp);
    return hipGetLastError();
}
extern "C" hipError_t ba_launch_seeding_sort(hipStream_t s, const ba::SeedingParams* sp) {
    k_seeding_sort<<<dim3(sp->n < 2048u ? sp->n : 2048u), dim3(SORT_THREADS), 0, s>>>(*sp);
    return hipGetLastError();
}
// The match's count pass (emit 0: hit_cnt) or emit pass (q_hit, r_hit, hit_len at hit_first).
extern "C" hipError_t ba_launch_seeding_match(hipStream_t s, const ba::SeedingParams* sp, int emit) {
    const uint32_t wgs = (sp->n + MATCH_WAVES - 1u) / MATCH_WAVES;
    const dim3 grid(wgs < 4096u ? wgs : 4096u), block(64 * MATCH_WAVES);
    if (emit) k_seeding_match<true><<<grid, block, 0, s>>>(*sp);
    else k_seeding_match<false><<<grid, block, 0, s>>>(*sp);
    return hipGetLastError();
}
