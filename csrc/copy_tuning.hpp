// Copy-kernel launch tuning, shared by kernels.hip (dispatch) and the gpu::
// layer (test/bench hooks). Production launches always use the process-wide
// default; the hooks may pass an explicit tuning so one process can reach
// every kernel variant and a capped grid at small sizes.
#pragma once

#include <cstddef>

namespace sw {

// Lane shape of the convert kernels for a 2-byte <-> 4-byte pair
// (kernels.hip "Convert family"): A is 8 elements per lane, B is 4.
// Default is what production runs.
enum class ConvertShape : int { Default = 0, A = 1, B = 2 };

// How the convert dispatch splits a message of n elements: `head` elements
// by the element kernel, `vectors` lanes of `lane_elems` elements by the
// vector kernel, `tail` elements by the element kernel; or, when no head
// co-aligns the two sides, everything by the element kernel (elem_only,
// tail == n).
struct ConvertPlan {
  bool elem_only;
  int lane_elems;
  size_t head, vectors, tail;
};

struct CopyTuning {
  size_t block_cap;     // max workgroups per launch (STARWAY_COPY_BLOCKS)
  size_t nt_threshold;  // bulk bytes at/above which the non-temporal kernels
                        // run (STARWAY_NT_THRESHOLD)
  int nt_unroll;        // >= 8 selects the x8 NT kernel (STARWAY_COPY_UNROLL)
  // Build one with designated initialisers (CopyTuning{.block_cap = n}): a
  // field left out is 0, which the hooks resolve to the process default.
  // Tile-contiguous streaming kernel (copy_stream.hpp).
  size_t stream_threshold = 0;  // bulk bytes at/above which it runs
                                // (STARWAY_STREAM_THRESHOLD)
  size_t stream_blocks = 0;     // its grid cap (STARWAY_STREAM_BLOCKS)
  // Accumulate kernels (reducing receive): bulk bytes at/above which the
  // SOURCE loads are non-temporal (STARWAY_ACCUM_NT_THRESHOLD). Its own
  // knob: the read-modify-write kernel crosses over far above the copies.
  size_t accum_nt_threshold = 0;
  // Convert kernels (converting receive): the lane shape, hooks only.
  ConvertShape convert_shape = ConvertShape::Default;
};

// Messages per batched small-message copy (k_copy_multi, begin_pull_multi):
// the size of the kernel's by-value descriptor array.
constexpr int kMultiMax = 8;

// stream_threshold value that no message reaches: the streaming kernel off.
constexpr size_t kStreamNever = ~(size_t)0;

// Which kernel an N-D copy (launch_copy_nd) runs. Auto is what
// production uses; the hooks force one so tests and benches reach both.
enum class CopyNdPath : int { Auto = 0, Generic = 1, Tiled = 2 };

// Index arithmetic of k_copy_nd and k_copy_indexed. Auto is what production
// uses: 32-bit wherever the granule count fits. Wide forces the 64-bit
// instantiations, which Auto reaches only past 2^32 - 1 granules; the hooks
// pass it so tests run them at every granule width on small messages.
enum class IndexWidth : int { Auto = 0, Wide = 1 };

// Environment-derived default (8192 blocks, 64 MiB, x4; streaming kernel
// from 64 MiB, 8192 blocks; accumulate NT source loads from 192 MiB), read
// once per process. Host-only: never
// touches the GPU.
const CopyTuning& default_copy_tuning();

}  // namespace sw
