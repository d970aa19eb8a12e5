// block_aligner_amd — the device helpers that minimizer seeding (ba_seeding.hip) and the reference index (ba_index.hip) share: the wave
// hand-offs, the hash and the two-bit codes of the rule ("Seeding"), a sketch's chunk of 64 windows and its selection, the
// binary search and the normalized bitonic network.
// Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ba {
namespace seed {

constexpr uint64_t NO_KEY = ~0ull;
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
// A, C, G, T in either case -> 0 .. 3, any other byte -> 4; rc: the complement. (Clearing bit 5 maps no byte but a and A onto A.)
__device__ __forceinline__ uint32_t two_bits(uint8_t c, bool rc) {
    c &= 0xdfu;
    const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    return rc && v < 4u ? 3u - v : v;
}
// code and order key (h << 32 | pos, all ones for an invalid k-mer or one past the end) of the k-mer over L.two[j .. j + k), position pos of
// a sequence with nk k-mers
__device__ __forceinline__ uint64_t kmer_key(const SketchLds& L, uint32_t j, uint32_t pos, uint32_t k, uint32_t nk, uint32_t& code) {
    uint32_t bad = 0;
    code = 0;
    for (uint32_t x = 0; x < k; x++) {
        const uint32_t v = L.two[j + x];
        bad |= v;
        code = code << 2 | (v & 3u);
    }
    return pos < nk && !(bad & 4u) ? (uint64_t)hash32(code) << 32 | pos : NO_KEY;
}
// One chunk of a sketch, the 64 windows from s0: the wave stages the two-bit codes of the chunk's bytes and a halo of k + w - 2 more in LDS
// (two(i): the code of byte i, 4 past the end), computes code and order key of the 63 + w k-mers under those windows, one or two per lane,
// and every lane takes the minimum of its window's w keys: all ones from window `end` on, and for a window without a valid k-mer.
template <class Two> __device__ __forceinline__ uint64_t chunk_minimizer(SketchLds& L, Two two, uint32_t s0, uint32_t end, uint32_t k, uint32_t w, uint32_t nk,
                                                                          uint32_t lane) {
    const uint32_t need_keys = 63u + w, need_bytes = need_keys + k - 1u;
    for (uint32_t b = lane; b < need_bytes; b += 64u) L.two[b] = (uint8_t)two(s0 + b);
    wave_sync();
    for (uint32_t j = lane; j < need_keys; j += 64u) {
        uint32_t code;
        L.key[j] = kmer_key(L, j, s0 + j, k, nk, code);
        L.code[j] = code;
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
// The same for canonical k-mers ("Both strands at once"): a staged k-mer also has a strand bit. At k = 16 a code fills all
// 32 bits, so the bit has a place of its own.
struct CanonLds {   // one wave's
    uint64_t key[CHUNK_KEYS];
    uint32_t code[CHUNK_KEYS];
    uint8_t two[CHUNK_BYTES];
    uint8_t strand[CHUNK_KEYS];
};
// kmer_key for the canonical code min(f, g) of the k-mer's forward code f and its reverse complement's g; strand: g < f. A palindrome
// (f == g) is invalid. The strand bit takes no part in the order key: of equal hashes the leftmost position wins, whatever the strands.
__device__ __forceinline__ uint64_t kmer_key_canon(const CanonLds& L, uint32_t j, uint32_t pos, uint32_t k, uint32_t nk, uint32_t& code, uint32_t& strand) {
    uint32_t bad = 0, f = 0;
    for (uint32_t x = 0; x < k; x++) {
        const uint32_t v = L.two[j + x];
        bad |= v;
        f = f << 2 | (v & 3u);
    }
    // g from f, once per k-mer: the complement is ~f; reversing all 32 bits brings the bases into reverse order at the top, each with its
    // two bits swapped, which the masks undo; the shift drops what ~ made of the bits above f's 2k
    uint32_t g = __brev(~f);
    g = ((g >> 1) & 0x55555555u) | ((g & 0x55555555u) << 1);
    g >>= 32u - 2u * k;
    strand = g < f ? 1u : 0u;
    code = strand ? g : f;
    return pos < nk && !(bad & 4u) && f != g ? (uint64_t)hash32(code) << 32 | pos : NO_KEY;
}
// chunk_minimizer over canonical k-mers: L.code and L.strand hold what the selected position's entry is made of.
template <class Two> __device__ __forceinline__ uint64_t chunk_minimizer_canon(CanonLds& L, Two two, uint32_t s0, uint32_t end, uint32_t k, uint32_t w,
                                                                                uint32_t nk, uint32_t lane) {
    const uint32_t need_keys = 63u + w, need_bytes = need_keys + k - 1u;
    for (uint32_t b = lane; b < need_bytes; b += 64u) L.two[b] = (uint8_t)two(s0 + b);
    wave_sync();
    for (uint32_t j = lane; j < need_keys; j += 64u) {
        uint32_t code, strand;
        L.key[j] = kmer_key_canon(L, j, s0 + j, k, nk, code, strand);
        L.code[j] = code;
        L.strand[j] = (uint8_t)strand;
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
