// Copy-kernel launch tuning, shared by kernels.hip (dispatch) and the gpu::
// layer (test/bench hooks). Production launches always use the process-wide
// default; the hooks may pass an explicit tuning so one process can reach
// every kernel variant and a capped grid at small sizes.
#pragma once

#include <cstddef>

namespace sw {

struct CopyTuning {
  size_t block_cap;     // max workgroups per launch (STARWAY_COPY_BLOCKS)
  size_t nt_threshold;  // bulk bytes at/above which the non-temporal kernels
                        // run (STARWAY_NT_THRESHOLD)
  int nt_unroll;        // >= 8 selects the x8 NT kernel (STARWAY_COPY_UNROLL)
};

// Which kernel an N-D copy (launch_copy_nd_tuned) runs. Auto is what
// production uses; the hooks force one so tests and benches reach both.
enum class CopyNdPath : int { Auto = 0, Generic = 1, Tiled = 2 };

// Environment-derived default (8192 blocks, 64 MiB, x4), read once per
// process. Host-only: never touches the GPU.
const CopyTuning& default_copy_tuning();

}  // namespace sw
