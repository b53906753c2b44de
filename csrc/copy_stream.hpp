// Tile-contiguous streaming copy for large co-aligned messages.
//
// The grid-stride kernels in kernels.hip keep a lane's unrolled accesses one
// grid stride apart (32 MiB at the default 8192-block cap), so the chip
// sweeps four read and four write windows at power-of-two distances. Here
// the message is cut into tiles of 256*U consecutive 16 B elements; lane t
// of a workgroup moves elements tile_base + j*256 + t for j < U, so each
// wave-instruction covers 1 KiB contiguous and the workgroup's U
// instructions cover the tile front to back. Tiles are dealt block-
// cyclically (workgroup b takes tiles b, b+G, b+2G, ...), so the resident
// workgroups together sweep ONE moving read window and ONE write window.
//
// The plan arithmetic (stream_plan / stream_block_tiles) is plain C++ so the
// host can test it without a GPU; the kernel itself needs hipcc.
#pragma once

#include <cstdint>

namespace sw {

constexpr uint32_t kStreamLanes = 256;      // workgroup size
constexpr uint32_t kStreamMaxGrid = 0x7fffffffu;

struct StreamPlan {
  uint64_t tile;        // 16 B elements per tile (256 * U)
  uint64_t full_tiles;  // tiles that run the unpredicated body
  uint64_t ragged;      // elements of the single bounds-checked last tile
  uint64_t tiles;       // full_tiles + (ragged ? 1 : 0)
  uint32_t grid;        // workgroups: min(tiles, stream_blocks)
};

// stream_blocks caps the grid; it must be >= 1. All indices are 64-bit: a
// tile index never exceeds n16 / tile and a byte offset is formed only as
// pointer arithmetic on 16 B elements.
constexpr StreamPlan stream_plan(uint64_t n16, uint32_t u,
                                 uint64_t stream_blocks) {
  StreamPlan p{};
  p.tile = (uint64_t)kStreamLanes * u;
  p.full_tiles = n16 / p.tile;
  p.ragged = n16 - p.full_tiles * p.tile;
  p.tiles = p.full_tiles + (p.ragged ? 1 : 0);
  uint64_t g = p.tiles < stream_blocks ? p.tiles : stream_blocks;
  if (g > kStreamMaxGrid) g = kStreamMaxGrid;
  p.grid = (uint32_t)g;
  return p;
}

// Tiles of workgroup b: first, first + grid, ..., last (count of them; 0
// means the block owns nothing, which only happens for b >= grid).
struct StreamBlockTiles {
  uint64_t first, last, count;
};

constexpr StreamBlockTiles stream_block_tiles(const StreamPlan& p,
                                              uint64_t b) {
  StreamBlockTiles r{b, b, 0};
  if (p.grid == 0 || b >= p.grid || b >= p.tiles) return r;
  r.count = (p.tiles - b + p.grid - 1) / p.grid;
  r.last = b + (r.count - 1) * p.grid;
  return r;
}

// Cache policy of the streaming kernel's loads / stores.
enum StreamPolicy : int {
  kStreamNtNt = 0,        // nt loads, nt stores
  kStreamPlainNt = 1,     // plain loads, nt stores
  kStreamPlainPlain = 2,  // plain loads, plain stores
};

}  // namespace sw

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace sw {

using stream_v4 = __attribute__((ext_vector_type(4))) unsigned int;

template <int POLICY>
__device__ __forceinline__ stream_v4 stream_ld(const stream_v4* p) {
  if constexpr (POLICY == kStreamNtNt) return __builtin_nontemporal_load(p);
  else return *p;
}
template <int POLICY>
__device__ __forceinline__ void stream_st(stream_v4 v, stream_v4* p) {
  if constexpr (POLICY == kStreamPlainPlain) *p = v;
  else __builtin_nontemporal_store(v, p);
}

// U elements per lane per tile; PREFETCH issues the loads of the workgroup's
// next tile before the stores of the current one (register double buffer).
template <int U, int POLICY, bool PREFETCH>
__global__ __launch_bounds__(256) void k_copy_stream(
    const stream_v4* __restrict__ src, stream_v4* __restrict__ dst,
    uint64_t n16) {
  constexpr uint64_t TILE = (uint64_t)kStreamLanes * U;
  const uint64_t G = gridDim.x;
  const uint64_t full = n16 / TILE;
  uint64_t t = blockIdx.x;
  if constexpr (!PREFETCH) {
    for (; t < full; t += G) {
      const uint64_t base = t * TILE + threadIdx.x;
      stream_v4 v[U];
#pragma unroll
      for (int j = 0; j < U; j++)
        v[j] = stream_ld<POLICY>(src + base + (uint64_t)j * kStreamLanes);
#pragma unroll
      for (int j = 0; j < U; j++)
        stream_st<POLICY>(v[j], dst + base + (uint64_t)j * kStreamLanes);
    }
  } else {
    if (t < full) {
      stream_v4 cur[U];
      uint64_t base = t * TILE + threadIdx.x;
#pragma unroll
      for (int j = 0; j < U; j++)
        cur[j] = stream_ld<POLICY>(src + base + (uint64_t)j * kStreamLanes);
      for (t += G; t < full; t += G) {
        const uint64_t nbase = t * TILE + threadIdx.x;
        stream_v4 nxt[U];
#pragma unroll
        for (int j = 0; j < U; j++)
          nxt[j] =
              stream_ld<POLICY>(src + nbase + (uint64_t)j * kStreamLanes);
#pragma unroll
        for (int j = 0; j < U; j++)
          stream_st<POLICY>(cur[j], dst + base + (uint64_t)j * kStreamLanes);
#pragma unroll
        for (int j = 0; j < U; j++) cur[j] = nxt[j];
        base = nbase;
      }
#pragma unroll
      for (int j = 0; j < U; j++)
        stream_st<POLICY>(cur[j], dst + base + (uint64_t)j * kStreamLanes);
    }
  }
  // t is now this workgroup's first tile index >= full. Exactly one
  // workgroup lands on the ragged tile (index == full) when there is one.
  if (t == full) {
    const uint64_t base = t * TILE + threadIdx.x;
#pragma unroll
    for (int j = 0; j < U; j++) {
      const uint64_t i = base + (uint64_t)j * kStreamLanes;
      if (i < n16) stream_st<POLICY>(stream_ld<POLICY>(src + i), dst + i);
    }
  }
}

// Launch one instantiation over the 16 B bulk [0, n16). src and dst are
// 16 B-aligned. stream_blocks >= 1.
template <int U, int POLICY, bool PREFETCH>
inline hipError_t launch_copy_stream(void* dst, const void* src, uint64_t n16,
                                     uint64_t stream_blocks,
                                     hipStream_t stream) {
  const StreamPlan p = stream_plan(n16, U, stream_blocks);
  if (p.grid == 0) return hipSuccess;
  hipLaunchKernelGGL((k_copy_stream<U, POLICY, PREFETCH>), dim3(p.grid),
                     dim3(kStreamLanes), 0, stream, (const stream_v4*)src,
                     (stream_v4*)dst, n16);
  return hipGetLastError();
}

}  // namespace sw
#endif  // __HIPCC__
