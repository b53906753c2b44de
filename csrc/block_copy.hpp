// Device-only: the block copy of one small message, shared by k_copy_multi
// (kernels.hip) and the inbox kernels (smallmsg.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sw {

// The whole 256-thread block copies `size` bytes: as 16 B vectors when the
// caller says it may (vec16: `size` and every pointer the caller cannot
// vouch for are multiples of 16), else as bytes. It only issues the
// accesses: draining them (s_waitcnt vmcnt(0)), the barrier and the
// release store that publishes the result stay in the calling kernel.
__device__ __forceinline__ void block_copy(uint8_t* dst, const uint8_t* src,
                                           uint32_t size, bool vec16) {
  if (!vec16) {
    for (uint32_t i = threadIdx.x; i < size; i += blockDim.x) dst[i] = src[i];
  } else {
    const uint4* s4 = (const uint4*)src;
    uint4* d4 = (uint4*)dst;
    for (uint32_t i = threadIdx.x; i < size / 16; i += blockDim.x)
      d4[i] = s4[i];
  }
}

}  // namespace sw
