// block_aligner_amd — the device helpers that minimizer seeding (ba_seeding.hip), the reference index (ba_index.hip) and both strands at once
// (ba_index_both.hip) share: the wave hand-offs and the persistent wave's work counter, the hash and the two-bit codes of the rule
// ("Seeding"), the sketch -- a chunk of 64 windows, its selection, the loop over a stretch of windows (sketch_windows) and
// the body of an index's sketch (index_sketch), each once for plain and for canonical k-mers (template <bool CANON>; "Both strands at
// once") --, the binary search and the normalized bitonic network.
// Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_index.h"

namespace ba {
namespace seed {

constexpr uint64_t NO_KEY = ~0ull;
constexpr uint32_t CHUNK_KEYS = 128, CHUNK_BYTES = 192;   // 64 windows: at most 63 + 64 k-mers over at most 63 + 64 + 15 bytes
static_assert(ba::INDEX_SPAN % 64u == 0u, "a span of an index's sketch is whole chunks");

// One wave's staging area. A canonical k-mer also has a strand bit: at k = 16 a code fills all 32 bits, so the bit has a place of its
// own, behind the plain fields.
template <bool CANON> struct SketchLdsOf;
template <> struct SketchLdsOf<false> {
    uint64_t key[CHUNK_KEYS];
    uint32_t code[CHUNK_KEYS];
    uint8_t two[CHUNK_BYTES];
};
template <> struct SketchLdsOf<true> : SketchLdsOf<false> {
    uint8_t strand[CHUNK_KEYS];
};
using SketchLds = SketchLdsOf<false>;
using CanonLds = SketchLdsOf<true>;

// lanes of one wave hand data to one another through LDS: program order is enough for the hardware, the compiler must keep it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t bcast(uint32_t x, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)lane); }
// A persistent wave's next work item: lane 0 takes it from the counter, which the host zeroes, and every lane gets it. (The barriers are
// convergence points: the wave is whole before and after the one lane's atomic.)
__device__ __forceinline__ uint32_t next_work(uint32_t* counter, uint32_t lane) {
    __builtin_amdgcn_wave_barrier();
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(counter, 1u);
    __builtin_amdgcn_wave_barrier();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}
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
__device__ __forceinline__ uint64_t wave_min64(uint64_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        x = o < x ? o : x;
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
// the first index in a[0 .. n) whose key is not below x
__device__ __forceinline__ uint32_t lower_bound(const uint64_t* a, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// A, C, G, T in either case -> 0 .. 3, any other byte -> 4; rc: the complement. (Clearing bit 5 maps no byte but a and A onto A.)
__device__ __forceinline__ uint32_t two_bits(uint8_t c, bool rc) {
    c &= 0xdfu;
    const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    return rc && v < 4u ? 3u - v : v;
}
// code and order key (h << 32 | pos, all ones for an invalid k-mer or one past the end) of the k-mer over L.two[j .. j + k), position pos of
// a sequence with nk k-mers. CANON: the code is min(f, g) of the k-mer's forward code f and its reverse complement's g; strand: g < f. A
// palindrome (f == g) is invalid. The strand bit takes no part in the order key: of equal hashes the leftmost position wins, whatever the
// strands.
template <bool CANON> __device__ __forceinline__ uint64_t kmer_key(const SketchLds& L, uint32_t j, uint32_t pos, uint32_t k, uint32_t nk, uint32_t& code,
                                                                    uint32_t& strand) {
    uint32_t bad = 0, f = 0;
    for (uint32_t x = 0; x < k; x++) {
        const uint32_t v = L.two[j + x];
        bad |= v;
        f = f << 2 | (v & 3u);
    }
    bool valid = pos < nk && !(bad & 4u);
    code = f;
    strand = 0;
    if constexpr (CANON) {
        // g from f, once per k-mer: the complement is ~f; reversing all 32 bits brings the bases into reverse order at the top, each with
        // its two bits swapped, which the masks undo; the shift drops what ~ made of the bits above f's 2k
        uint32_t g = __brev(~f);
        g = ((g >> 1) & 0x55555555u) | ((g & 0x55555555u) << 1);
        g >>= 32u - 2u * k;
        strand = g < f ? 1u : 0u;
        code = strand ? g : f;
        valid = valid && f != g;
    }
    return valid ? (uint64_t)hash32(code) << 32 | pos : NO_KEY;
}
// One chunk of a sketch, the 64 windows from s0: the wave stages the two-bit codes of the chunk's bytes and a halo of k + w - 2 more in LDS
// (two(i): the code of byte i, 4 past the end), computes code and order key of the 63 + w k-mers under those windows, one or two per lane,
// and every lane takes the minimum of its window's w keys: all ones from window `end` on, and for a window without a valid k-mer. L.code
// (and L.strand) hold what the selected position's entry is made of.
template <bool CANON, class Two> __device__ __forceinline__ uint64_t chunk_minimizer(SketchLdsOf<CANON>& L, Two two, uint32_t s0, uint32_t end, uint32_t k,
                                                                                      uint32_t w, uint32_t nk, uint32_t lane) {
    const uint32_t need_keys = 63u + w, need_bytes = need_keys + k - 1u;
    for (uint32_t b = lane; b < need_bytes; b += 64u) L.two[b] = (uint8_t)two(s0 + b);
    wave_sync();
    for (uint32_t j = lane; j < need_keys; j += 64u) {
        uint32_t code, strand;
        L.key[j] = kmer_key<CANON>(L, j, s0 + j, k, nk, code, strand);
        L.code[j] = code;
        if constexpr (CANON) L.strand[j] = (uint8_t)strand;
    }
    wave_sync();
    uint64_t m = NO_KEY;
    if (s0 + lane < end)
        for (uint32_t x = 0; x < w; x++) {
            const uint64_t c = L.key[lane + x];
            m = c < m ? c : m;
        }
    return m;
}
// A window's minimizer is selected when it differs from the window's before it -- the minimizers of consecutive windows never go back --;
// prev: the minimizer of the window before the chunk, and then of the chunk's last window.
__device__ __forceinline__ bool chunk_select(uint64_t m, uint64_t& prev, uint32_t lane) {
    const uint32_t bl = (uint32_t)__shfl_up((int)(uint32_t)m, 1, 64), bh = (uint32_t)__shfl_up((int)(uint32_t)(m >> 32), 1, 64);
    const uint64_t before = lane ? (uint64_t)bh << 32 | bl : prev;
    prev = (uint64_t)bcast((uint32_t)(m >> 32), 63) << 32 | bcast((uint32_t)m, 63);
    return m != NO_KEY && m != before;
}
// The sketch of the windows [first, last), 64 at a time: the selected minimizers are compacted by a ballot and a running count, and
// put(at, code, low) writes the at-th of them: low is its position, with the strand in bit 31 when CANON. prev: the minimizer of window
// first - 1, all ones when there is none. -> how many were selected (the count pass, EMIT false, writes nothing).
template <bool CANON, bool EMIT, class Two, class Put>
__device__ __forceinline__ uint32_t sketch_windows(SketchLdsOf<CANON>& L, Two two, uint32_t first, uint32_t last, uint32_t k, uint32_t w, uint32_t nk,
                                                   uint64_t prev, uint32_t lane, Put put) {
    uint32_t count = 0;
    for (uint32_t s0 = first; s0 < last; s0 += 64u) {
        const uint64_t m = chunk_minimizer<CANON>(L, two, s0, last, k, w, nk, lane);   // (a window past the last one selects nothing)
        const bool take = chunk_select(m, prev, lane);
        const uint64_t ballot = __ballot(take);
        if (EMIT && take) {
            const uint32_t pos = (uint32_t)m;
            uint32_t low = pos;
            if constexpr (CANON) low |= (uint32_t)L.strand[pos - s0] << 31;
            put(count + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)), L.code[pos - s0], low);
        }
        count += (uint32_t)__popcll(ballot);
        wave_sync();   // the next chunk overwrites what this one read
    }
    return count;
}
// The sketch of an index (k_index_sketch, k_both_index_sketch), a persistent wave's count pass or emit pass. A work item is a span of
// INDEX_SPAN windows of one sequence, taken from the work counter. The seam: a window's minimizer is selected when it differs from the
// window's before it, so a span that does not start its sequence first computes the minimizer of the window before its first one from
// the w k-mers under that window -- all ones when none of them is valid, which is also what a sequence's first window compares with.
// The entries are written as keys code << 32 | low, in position order. Several sequences lie end to end in one frame; the host numbers
// every sequence's spans from seq_span[s], the wave finds its span's sequence by a lower bound over those, and every byte outside that
// sequence reads as invalid: one reference is the case n_seqs = 1, with the same arithmetic.
template <bool CANON, bool EMIT> __device__ __forceinline__ void index_sketch(const ba::IndexParams& ip, SketchLdsOf<CANON>& L) {
    const uint32_t lane = threadIdx.x & 63u, k = ip.k, w = ip.w;
    for (;;) {
        const uint32_t t = next_work(ip.counter, lane);
        if (t >= ip.n_spans) break;
        // the span's sequence: the last one whose first span is t or before it (a sequence without a k-mer has no span, so it is never that)
        const uint32_t sq = lower_bound(ip.seq_span, ip.n_seqs + 1u, (uint64_t)t + 1u) - 1u;
        const uint32_t S = (uint32_t)ip.seq_start[sq], E = (uint32_t)ip.seq_start[sq + 1u];   // its bytes, in the index's frame (E - S >= k)
        const uint32_t nk = E - k + 1u;   // one past its last k-mer; positions, k-mers and windows are numbered in the index's frame from here on
        const uint32_t nw = nk - S > w ? nk - w + 1u : S + 1u;   // one past its last window
        const auto two = [&](uint32_t i) { return i >= S && i < E ? two_bits(ip.ref[i], false) : 4u; };   // (no byte of a neighbour)
        const uint32_t first = S + (t - (uint32_t)ip.seq_span[sq]) * ba::INDEX_SPAN, last = first + ba::INDEX_SPAN < nw ? first + ba::INDEX_SPAN : nw;
        uint64_t prev = NO_KEY;   // the minimizer of the window before the span
        if (first != S) {         // the seam: window first - 1 lies over the k-mers first - 1 .. first + w - 2 (the sequence has more than w here)
            for (uint32_t b = lane; b < w + k - 1u; b += 64u) L.two[b] = (uint8_t)two(first - 1u + b);
            wave_sync();
            uint32_t code, strand;
            prev = wave_min64(lane < w ? kmer_key<CANON>(L, lane, first - 1u + lane, k, nk, code, strand) : NO_KEY);
            wave_sync();   // the first chunk overwrites what this read
        }
        const uint64_t out0 = EMIT ? ip.span_first[t] : 0ull;
        // (a window past the span's last one is the next span's)
        const uint32_t count = sketch_windows<CANON, EMIT>(L, two, first, last, k, w, nk, prev, lane,
                                                           [&](uint32_t at, uint32_t code, uint32_t low) { ip.unsorted[out0 + at] = (uint64_t)code << 32 | low; });
        if (!EMIT && lane == 0) ip.span_cnt[t] = count;
    }
}
// one compare-exchange of the sort: ascending, and skipped when the partner lies past the end
__device__ __forceinline__ void exchange(uint64_t* a, uint32_t i, uint32_t l, uint32_t n) {
    if (l < n) {
        const uint64_t x = a[i], y = a[l];
        if (x > y) { a[i] = y; a[l] = x; }
    }
}
// The normalized bitonic network over a[0 .. n), in LDS or in global memory, by all THREADS threads of the workgroup. Blocks of 2, 4, 8, ...:
// first every entry against its mirror image in the block, then halves of halves at distance j.
template <uint32_t THREADS> __device__ __forceinline__ void sort_network(uint64_t* a, uint32_t n) {
    uint32_t lg = 1;
    while ((1ull << lg) < n) lg++;
    const uint32_t pairs = 1u << (lg - 1u);
    for (uint32_t b = 1; b <= lg; b++) {   // blocks of 1 << b entries
        for (uint32_t t = threadIdx.x; t < pairs; t += THREADS) {
            const uint32_t i = (t >> (b - 1u)) << b | (t & ((1u << (b - 1u)) - 1u));
            exchange(a, i, i ^ ((1u << b) - 1u), n);
        }
        __syncthreads();
        for (uint32_t lj = b - 1u; lj-- > 0u;) {   // distance 1 << lj
            for (uint32_t t = threadIdx.x; t < pairs; t += THREADS) {
                const uint32_t i = (t >> lj) << (lj + 1u) | (t & ((1u << lj) - 1u));
                exchange(a, i, i + (1u << lj), n);
            }
            __syncthreads();
        }
    }
}

}  // namespace seed
}  // namespace ba
