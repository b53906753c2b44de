// Test/bench hooks of the GPU layer: synchronous entry points behind the
// `_`-prefixed functions of starway_amd._core (module_hooks.cpp). Defined
// in gpu.cpp and smallmsg.hip, next to the statics they use; the engine
// calls none of them, so the GPU-less stub (gpu_stub.cpp) has none either.
#pragma once

#include "core.hpp"

namespace sw {
namespace gpu {

// Synchronous copy-kernel launches on the pull stream. A zero field in
// `tuning` / a zero block_cap means the default tuning.
CopyTuning copy_tuning();  // the default; never touches the GPU
// Elements per lane per tile (U) of the production streaming kernel
// (copy_stream.hpp); a compile-time constant, never touches the GPU.
int copy_stream_unroll();
bool copy_device_sync(void* dst, const void* src, size_t n, int device,
                      const CopyTuning& tuning, std::string* err);
bool copy_strided_sync(void* dst, uint64_t dst_stride, const void* src,
                       uint64_t src_stride, uint64_t rows, uint64_t row_bytes,
                       int device, size_t block_cap, std::string* err);
// N-D copy (k_copy_nd / k_copy_nd_tile). Both layouts describe `bytes`
// message bytes. *ineligible is set when path == Tiled was asked for a
// pair outside the transpose family (nothing is launched then). `width`
// other than Auto forces k_copy_nd's 64-bit index instantiation.
bool copy_nd_sync(void* dst, const Layout& dst_layout, const void* src,
                  const Layout& src_layout, uint64_t bytes, int device,
                  size_t block_cap, CopyNdPath path, IndexWidth width,
                  bool* ineligible, std::string* err);
// Tile extent (elements, both axes) of k_copy_nd_tile per element size;
// a compile-time constant of the kernels, 0 for an unsupported size.
int copy_nd_tile_extent(int elem_bytes);
// Indexed copy (k_copy_indexed) of `bytes` message bytes. A side whose list
// is off is one dense run; at least one side is indexed. The lists are
// uploaded on the pull stream ahead of the kernel, as in production.
bool copy_index_sync(void* dst, const IndexRef& dst_index, const void* src,
                     const IndexRef& src_index, uint64_t bytes, int device,
                     size_t block_cap, IndexWidth width, std::string* err);
struct CopyDesc {
  void* dst;
  const void* src;
  uint64_t bytes;
};
bool copy_multi_sync(const CopyDesc* descs, int n, int device,
                     std::string* err);
// The accumulate kernels (launch_accum): dst[i] += src[i] over
// nbytes / elem_size(dtype) elements. Refuses pointers or a length that
// are not multiples of the element size.
bool accum_sync(void* dst, const void* src, size_t nbytes, ElemType dtype,
                int device, const CopyTuning& tuning, std::string* err);
// The convert kernels (launch_convert): dst[i] = dst_type(src[i]), or with
// `accumulate` dst_type(float(dst[i]) + float(src[i])), over n_elems
// elements. tuning.convert_shape picks the lane shape. The caller has
// checked the types and each pointer's alignment to its element size.
bool convert_sync(void* dst, ElemType dst_type, const void* src,
                  ElemType src_type, size_t n_elems, bool accumulate,
                  int device, const CopyTuning& tuning, std::string* err);
// launch_convert's split of such a message (kernels.hpp); host only.
ConvertPlan convert_plan(uintptr_t dst, ElemType dst_type, uintptr_t src,
                         ElemType src_type, size_t n_elems,
                         ConvertShape shape);
// The lane shape production launches run, and a bench's override of it
// (Default restores the production shape). Host only.
ConvertShape convert_default_shape();
void set_convert_default_shape(ConvertShape shape);

// The inbox kernels (smallmsg.hip). These drive the kernels through the
// host functions the engine uses (same-process push, lane 0) and wait
// under a host deadline; none of them launches a kernel of its own.
bool inbox_ring_read(const InboxInfo& ring, uint8_t* out, std::string* err);
bool inbox_ring_write(const InboxInfo& ring, uint64_t offset,
                      const uint8_t* data, uint64_t n, std::string* err);
// One k_inbox_push launch, polled to completion, ticket freed.
bool inbox_push_sync(const InboxInfo& ring, const PushMsg* msgs, int n,
                     int run_device, std::string* err);
// One k_inbox_unpack launch. status[i] is the kernel's result word (1 ok /
// 2 payload never arrived); bounce[i] holds the pinned staging bytes of a
// message whose dst was null and is empty otherwise.
bool inbox_unpack_sync(const InboxInfo& ring, const UnpackMsg* msgs, int n,
                       int* status, std::vector<uint8_t>* bounce,
                       std::string* err);
// arm_recv, with the cancel word optionally set BEFORE the launch is
// enqueued (the kernel then starts canceled, whatever the queue does).
void* arm_begin(const InboxInfo& ring, uint64_t expect_seq, uint64_t tag,
                uint64_t mask, uint8_t* dst, uint64_t max_size,
                unsigned spin_iters, bool precancel, std::string* err);
// Wait for the kernel's verdict, then free the ticket. Past the deadline:
// cancel, wait 100 ms, and leak the cell if the kernel still has not
// reported (false; the ticket is gone either way).
bool arm_end(void* ticket, int* status, uint64_t* size, std::string* err);

}  // namespace gpu
}  // namespace sw
