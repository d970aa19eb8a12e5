// block_aligner_amd — device helpers that the exact kernels share (ba_exact.hip, ba_exact_modes.hip): the wave shifts and reductions of the
// skewed sweep and the split score lookup of the sequence kinds.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_exact.h"

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

}  // namespace
