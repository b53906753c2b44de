// Element type of a reducing receive: what the accumulate kernels
// (kernels.hip) add, dst[i] = dst[i] + src[i]. F16/BF16 add in fp32 and
// round once, to nearest even; I32 wraps. Shared by the engine's BufferRef
// (core.hpp), the gpu:: layer and the kernels.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sw {

enum class ElemType : uint8_t { None = 0, F32, F16, BF16, I32 };

inline size_t elem_size(ElemType t) {
  switch (t) {
    case ElemType::F32:
    case ElemType::I32: return 4;
    case ElemType::F16:
    case ElemType::BF16: return 2;
    case ElemType::None: break;
  }
  return 0;
}

}  // namespace sw
