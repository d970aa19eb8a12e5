// The sort of a reference index's keys (ba_ref_index_create, ba_host.cpp): a one-time build step, not the hot path, so it is rocPRIM's radix
// sort. A translation unit of its own: the resource report of the hand-written kernels (ba_index.hip) stays free of library kernels.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "ba_launch.h"

// Sort in[0 .. n) by its low `bits` bits into out. With temp = nullptr only *temp_bytes is set: the two calls of rocPRIM's pattern.
extern "C" hipError_t ba_launch_index_sort(hipStream_t s, const uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits, void* temp, size_t* temp_bytes) {
    return rocprim::radix_sort_keys(temp, *temp_bytes, in, out, (size_t)n, 0u, bits, s);
}
