// Everything kernels.hip exports: the host-side launchers of the gfx950
// copy and accumulate kernels. Included by kernels.hip itself, so a
// declaration that drifts from its definition does not compile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "copy_tuning.hpp"
#include "elem_type.hpp"
#include "index.hpp"
#include "layout.hpp"

namespace sw {

// One message of a batched small-message copy (k_copy_multi): up to
// kMultiMax (copy_tuning.hpp) per launch, one block per message.
struct MultiCopyDesc {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t bytes;
};
// Callers validate 1 <= n <= kMultiMax and bytes < 2^32.
hipError_t launch_copy_multi(const MultiCopyDesc* descs, int n,
                             hipStream_t stream);

// same_device: src and dst live on the GPU that runs the kernel. Only then
// may the copy take the streaming route (see launch_copy in kernels.hip).
hipError_t launch_copy(void* dst, const void* src, size_t bytes,
                       hipStream_t stream, bool same_device);
// The flat dispatch itself, under any tuning (hooks, bin/copy_bench).
hipError_t launch_copy_tuned(void* dst, const void* src, size_t bytes,
                             hipStream_t stream,
                             const CopyTuning& t = default_copy_tuning());
// Elements per lane per tile (U) of the production streaming kernel.
int copy_stream_unroll();

hipError_t launch_copy_strided(void* dst, uint64_t dst_stride,
                               const void* src, uint64_t src_stride,
                               uint64_t rows, uint64_t row_bytes,
                               hipStream_t stream,
                               const CopyTuning& t = default_copy_tuning());

// Both layouts describe `bytes` message bytes.
hipError_t launch_copy_nd(void* dst, const Layout& dst_layout,
                          const void* src, const Layout& src_layout,
                          uint64_t bytes, hipStream_t stream,
                          const CopyTuning& t = default_copy_tuning(),
                          CopyNdPath path = CopyNdPath::Auto,
                          IndexWidth width = IndexWidth::Auto);
// Tile extent (elements, both axes) of k_copy_nd_tile per element size; 0
// for an unsupported size.
int copy_nd_tile_extent(int elem_bytes);
// Whether the tiled kernel serves this pair of layouts and pointers.
bool copy_nd_tile_eligible(const Layout& src_layout, const Layout& dst_layout,
                           const void* src, const void* dst);

// Indexed copy (index.hpp) of `bytes` message bytes: message byte m lies at
// base + index[m / slice_bytes] * stride + m % slice_bytes on a side with a
// (device) index list and at base + m on a side whose list is null. At
// least one side is indexed; each indexed side's slices add up to `bytes`.
hipError_t launch_copy_indexed(void* dst, const IndexSide& dst_side,
                               const void* src, const IndexSide& src_side,
                               uint64_t bytes, hipStream_t stream,
                               const CopyTuning& t = default_copy_tuning(),
                               IndexWidth width = IndexWidth::Auto);

// dst[i] += src[i]; both pointers aligned to the element size, bytes a
// multiple of it, no overlap.
hipError_t launch_accum(void* dst, const void* src, size_t bytes,
                        ElemType dtype, hipStream_t stream,
                        const CopyTuning& t = default_copy_tuning());

// Converting copy: dst[i] = dst_type(src[i]), or with `accumulate`
// dst[i] = dst_type(float(dst[i]) + float(src[i])), over n_elems elements,
// through fp32 and rounded once. The types are two different ones of F32,
// F16, BF16; each pointer is aligned to its own element size; no overlap.
// t.convert_shape picks the lane shape of a 2-byte <-> 4-byte pair.
hipError_t launch_convert(void* dst, ElemType dst_type, const void* src,
                          ElemType src_type, size_t n_elems, bool accumulate,
                          hipStream_t stream,
                          const CopyTuning& t = default_copy_tuning());
// How launch_convert splits a message (ConvertPlan, copy_tuning.hpp).
ConvertPlan convert_plan(uintptr_t dst, ElemType dst_type, uintptr_t src,
                         ElemType src_type, size_t n_elems,
                         ConvertShape shape = ConvertShape::Default);
// What ConvertShape::Default resolves to: the production shape, unless a
// bench has set another (Default sets it back). Host only.
ConvertShape convert_default_shape();
void set_convert_default_shape(ConvertShape shape);

}  // namespace sw
