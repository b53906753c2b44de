// gfx950 (CDNA4 / MI355X) data-movement kernels for starway_amd.
//
// These are the hand-written copy kernels that replace what UCX's internal
// copy paths did for the reference (ucp_tag_send/recv delivery). A tagged
// message delivery is one device-side copy: local HBM->HBM on one GPU, or a
// peer read over xGMI when src is another GPU's memory (hipIpc-mapped or
// same-process peer pointer).
//
// Design (per MI355X microarch):
//  * 64-wide wavefronts; 256-thread workgroups (4 waves)
//  * 16 B/lane vector moves (global_load_dwordx4 / global_store_dwordx4):
//    1 KiB per wave-instruction — the measured-fastest HBM streaming shape
//    (float4 copy reaches 6.29 TB/s read on this chip)
//  * grid-stride loop sized >> 256 workgroups so all 8 XCDs fill
//  * unroll by 4 so each thread has 4 independent loads in flight (latency
//    hiding without LDS staging — a pure stream copy has no reuse, so LDS
//    would only add a round trip)
//  * non-temporal variants for large messages: a message buffer is read and
//    written exactly once, so polluting L2/LLC with it costs other traffic.
//  * same-device copies of 64 MiB and more take the tile-contiguous
//    streaming kernel (copy_stream.hpp) instead: the grid-stride loops
//    above keep a lane's unrolled accesses one grid stride (32 MiB at 8192
//    blocks) apart, the streaming kernel sweeps one contiguous window.
//    Measured at 256 MiB: 84.3 us against 104.6 us, 6.37 against 5.13 TB/s
//    of HBM traffic (docs/benchmark.md "Streaming copy").
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "block_copy.hpp"
#include "copy_stream.hpp"
#include "kernels.hpp"

namespace sw {

// The builtin non-temporal accesses want a native vector type, not
// HIP_vector_type.
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

// 16 B load and store, plain or non-temporal. Non-temporal is for data that
// is touched exactly once (messages past the LLC-thrash threshold, a large
// accumulate source) and would otherwise sweep the cache.
template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void st16(u32x4 v, u32x4* p) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// The access type of a G-byte granule.
template <int G> struct GranuleT;
template <> struct GranuleT<16> { using type = uint4; };
template <> struct GranuleT<8> { using type = uint2; };
template <> struct GranuleT<4> { using type = uint32_t; };
template <> struct GranuleT<2> { using type = uint16_t; };
template <> struct GranuleT<1> { using type = uint8_t; };

// ---------------------------------------------------------------------------
// 16B-vector bulk copy (both pointers 16B-aligned), grid-stride, U
// independent elements in flight per thread per iteration. Production runs
// <4, false>, <4, true> (bypass-cache hints on both sides, from
// nt_threshold) and <8, true> (nt_unroll >= 8).
//
// One iteration is a pack expansion, not a `#pragma unroll` loop: the loop
// is unrolled late in the compiler and comes out with other address
// arithmetic and, at U = 8, another interleaving of loads and stores than
// the straight-line statements the measurements in docs/benchmark.md were
// taken with. The pack is straight-line from the start.
// ---------------------------------------------------------------------------
template <bool NT, size_t... K>
__device__ __forceinline__ void copy16_each(const u32x4* src, u32x4* dst,
                                            size_t i, size_t stride,
                                            std::index_sequence<K...>) {
  u32x4 v[] = {ld16<NT>(&src[i + K * stride])...};
  (st16<NT>(v[K], &dst[i + K * stride]), ...);
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void k_copy_b128(
    const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  while (i + (U - 1) * stride < n16) {
    copy16_each<NT>(src, dst, i, stride, std::make_index_sequence<U>{});
    i += U * stride;
  }
  for (; i < n16; i += stride) {
    u32x4 v = ld16<NT>(&src[i]);
    st16<NT>(v, &dst[i]);
  }
}

// Element-granularity fallback: G = 1 for arbitrary (mis)alignment, heads
// and tails; G = 4 when both sides are 4B-co-aligned but not 16B.
template <int G>
__global__ __launch_bounds__(256) void k_copy_elem(
    const typename GranuleT<G>::type* __restrict__ src,
    typename GranuleT<G>::type* __restrict__ dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// Strided (2D) pack/unpack copy: row r of the message lives at
// src + r*src_stride and lands at dst + r*dst_stride; rows are dense runs of
// row_n G-byte granules (G = 16 when everything is 16B-aligned, else 1).
// Used for non-contiguous device tensors (e.g. torch slices) so they move
// without a .contiguous() staging pass. Lanes walk granules in row-major
// message order, so global accesses stay coalesced within each row.
// ---------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void k_copy_strided(
    const uint8_t* __restrict__ src, uint64_t src_stride,
    uint8_t* __restrict__ dst, uint64_t dst_stride, uint64_t rows,
    uint64_t row_n) {
  using V = typename GranuleT<G>::type;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t total = (size_t)rows * row_n;
  for (; i < total; i += stride) {
    size_t r = i / row_n;
    size_t c = i - r * row_n;
    *(V*)(dst + r * dst_stride + c * G) =
        *(const V*)(src + r * src_stride + c * G);
  }
}

// ---------------------------------------------------------------------------
// Batched small-message copy: up to kMultiMax messages per launch, one
// block per message (messages <= ~64 KiB). Amortizes the launch + event
// cost that dominates small-message rate (measured: raw engine pipeline
// sustains 600k msgs/s on host buffers but 85k with one launch+event per
// device message).
// ---------------------------------------------------------------------------
struct MultiCopyArgs {
  MultiCopyDesc d[kMultiMax];
  int n;
};

__global__ __launch_bounds__(256) void k_copy_multi(MultiCopyArgs args) {
  const MultiCopyDesc& m = args.d[blockIdx.x];
  block_copy(m.dst, m.src, m.bytes,
             ((uintptr_t)m.src & 15) == 0 && ((uintptr_t)m.dst & 15) == 0 &&
                 (m.bytes & 15) == 0);
}

hipError_t launch_copy_multi(const MultiCopyDesc* descs, int n,
                             hipStream_t stream) {
  MultiCopyArgs args;
  for (int i = 0; i < n; i++) args.d[i] = descs[i];
  args.n = n;
  hipLaunchKernelGGL(k_copy_multi, dim3(n), dim3(256), 0, stream, args);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Host-side dispatch
// ---------------------------------------------------------------------------

// The one streaming instantiation production runs, and its defaults: the
// winner of the alternating sweep recorded in docs/benchmark.md ("Streaming
// copy"). bin/copy_bench instantiates the whole matrix.
constexpr int kStreamProdU = 4;
constexpr int kStreamProdPolicy = kStreamNtNt;
constexpr bool kStreamProdPrefetch = false;
constexpr size_t kStreamDefaultThreshold = (size_t)64 << 20;
constexpr size_t kStreamDefaultBlocks = 8192;
// Accumulate kernels: non-temporal source loads from this size. Swept on
// MI355X, same device, both variants forced, fp32 / bf16, median of 9
// rounds x 10 calls (docs/benchmark.md "Reducing receive"): the plain
// loads are faster up to 128 MiB (by 4-6 % at 64 MiB), the two are level
// at 160 MiB (within 2 % either way), and from 192 MiB the non-temporal
// loads win with the ranges apart (6-7 % at 192 MiB, 13-14 % at 224 MiB,
// 20-24 % at 256 MiB). 192 MiB is the smallest measured size where they
// win for both types.
constexpr size_t kAccumNtDefaultThreshold = (size_t)192 << 20;

// Empty or unset gives the default, anything else is read as decimal.
static size_t env_size(const char* name, size_t dflt) {
  const char* v = getenv(name);
  return v && *v ? (size_t)strtoull(v, nullptr, 10) : dflt;
}

const CopyTuning& default_copy_tuning() {
  // Read once per process; the variables exist for on-box sweeps
  // (scripts/copy_tune.sh).
  static const CopyTuning t = [] {
    CopyTuning d;
    d.block_cap = env_size("STARWAY_COPY_BLOCKS", 8192);
    // NT past 64 MiB: the copy would otherwise sweep the 256 MiB LLC.
    d.nt_threshold = env_size("STARWAY_NT_THRESHOLD", (size_t)64 << 20);
    const char* v = getenv("STARWAY_COPY_UNROLL");
    d.nt_unroll = v && *v ? atoi(v) : 4;
    d.stream_threshold =
        env_size("STARWAY_STREAM_THRESHOLD", kStreamDefaultThreshold);
    d.stream_blocks = env_size("STARWAY_STREAM_BLOCKS", kStreamDefaultBlocks);
    d.accum_nt_threshold =
        env_size("STARWAY_ACCUM_NT_THRESHOLD", kAccumNtDefaultThreshold);
    return d;
  }();
  return t;
}

static inline int copy_grid(size_t work_items, size_t cap) {
  // >> 256 WGs to fill 8 XCDs x 32 CUs; cap so tiny copies stay one-wave-ish.
  size_t blocks = (work_items + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > cap) blocks = cap;
  return (int)blocks;
}

// A runtime granule (1/2/4/8/16 bytes; anything else counts as 1) as a
// compile-time constant: f(std::integral_constant<int, G>{}).
template <class F>
static void with_granule(uint64_t g, F&& f) {
  switch (g) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
}

// Index type of a kernel that divides by quantities the count `n` bounds:
// f(uint32_t{}) where every value fits, else f(uint64_t{}). 64-bit division
// costs several times the 32-bit one on gfx950. Any width but Auto takes
// the 64-bit form whatever the count (test hooks only).
template <class F>
static void with_index_width(uint64_t n, IndexWidth width, F&& f) {
  if (width == IndexWidth::Auto && n <= UINT32_MAX) f(uint32_t{});
  else f(uint64_t{});
}

// The co-aligned split of a run of `bytes` at address p (the other side has
// the same p & 15): `head` bytes up to the next 16B boundary, n16 whole 16 B
// vectors, `tail` bytes.
struct Split16 {
  size_t head, n16, tail;
};
static inline Split16 split16(uintptr_t p, size_t bytes) {
  size_t head = (16 - (p & 15)) & 15;
  if (head > bytes) head = bytes;
  return {head, (bytes - head) / 16, (bytes - head) & 15};
}

int copy_stream_unroll() { return kStreamProdU; }

hipError_t launch_copy_tuned(void* dst, const void* src, size_t bytes,
                             hipStream_t stream, const CopyTuning& t) {
  if (bytes == 0) return hipSuccess;
  const size_t cap = t.block_cap;
  uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
  if ((s & 15) == (d & 15)) {
    // Co-aligned: byte head, vector bulk, byte tail.
    const auto [head, n16, tail] = split16(s, bytes);
    if (head)
      hipLaunchKernelGGL(k_copy_elem<1>, dim3(1), dim3(64), 0, stream,
                         (const uint8_t*)s, (uint8_t*)d, head);
    s += head;
    d += head;
    const u32x4* s16 = (const u32x4*)s;
    u32x4* d16 = (u32x4*)d;
    if (n16) {
      if (n16 * 16 >= t.stream_threshold) {
        hipError_t e =
            launch_copy_stream<kStreamProdU, kStreamProdPolicy,
                               kStreamProdPrefetch>(
                d16, s16, n16, t.stream_blocks ? t.stream_blocks : 1, stream);
        if (e != hipSuccess) return e;
      } else if (bytes - head >= t.nt_threshold) {
        if (t.nt_unroll >= 8)
          hipLaunchKernelGGL((k_copy_b128<8, true>),
                             dim3(copy_grid(n16 / 8 + 1, cap)), dim3(256), 0,
                             stream, s16, d16, n16);
        else
          hipLaunchKernelGGL((k_copy_b128<4, true>),
                             dim3(copy_grid(n16 / 4 + 1, cap)), dim3(256), 0,
                             stream, s16, d16, n16);
      } else {
        hipLaunchKernelGGL((k_copy_b128<4, false>),
                           dim3(copy_grid(n16 / 4 + 1, cap)), dim3(256), 0,
                           stream, s16, d16, n16);
      }
    }
    if (tail)
      hipLaunchKernelGGL(k_copy_elem<1>, dim3(1), dim3(64), 0, stream,
                         (const uint8_t*)(s16 + n16), (uint8_t*)(d16 + n16),
                         tail);
  } else if ((s & 3) == (d & 3) && (s & 3) == 0 && (bytes & 3) == 0) {
    size_t n4 = bytes / 4;
    hipLaunchKernelGGL(k_copy_elem<4>, dim3(copy_grid(n4 / 4 + 1, cap)),
                       dim3(256), 0, stream, (const uint32_t*)src,
                       (uint32_t*)dst, n4);
  } else {
    hipLaunchKernelGGL(k_copy_elem<1>, dim3(copy_grid(bytes / 16 + 1, cap)),
                       dim3(256), 0, stream, (const uint8_t*)src,
                       (uint8_t*)dst, bytes);
  }
  return hipGetLastError();
}

hipError_t launch_copy(void* dst, const void* src, size_t bytes,
                       hipStream_t stream, bool same_device) {
  if (same_device) return launch_copy_tuned(dst, src, bytes, stream);
  // The streaming route was measured only for same-device copies; nothing
  // here can measure a pull over xGMI, and an unmeasured path does not
  // change: a cross-device pull keeps the grid-stride kernels.
  CopyTuning t = default_copy_tuning();
  t.stream_threshold = kStreamNever;
  return launch_copy_tuned(dst, src, bytes, stream, t);
}

hipError_t launch_copy_strided(void* dst, uint64_t dst_stride,
                               const void* src, uint64_t src_stride,
                               uint64_t rows, uint64_t row_bytes,
                               hipStream_t stream, const CopyTuning& t) {
  if (rows == 0 || row_bytes == 0) return hipSuccess;
  const size_t cap = t.block_cap;
  uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
  bool vec = (s & 15) == 0 && (d & 15) == 0 && (src_stride & 15) == 0 &&
             (dst_stride & 15) == 0 && (row_bytes & 15) == 0;
  if (vec) {
    uint64_t row_n16 = row_bytes / 16;
    size_t total = (size_t)rows * row_n16;
    hipLaunchKernelGGL(k_copy_strided<16>,
                       dim3(copy_grid(total / 4 + 1, cap)), dim3(256), 0,
                       stream, (const uint8_t*)src, src_stride, (uint8_t*)dst,
                       dst_stride, rows, row_n16);
  } else {
    size_t total = (size_t)rows * row_bytes;
    hipLaunchKernelGGL(k_copy_strided<1>,
                       dim3(copy_grid(total / 16 + 1, cap)), dim3(256), 0,
                       stream, (const uint8_t*)src, src_stride, (uint8_t*)dst,
                       dst_stride, rows, row_bytes);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// N-D pack/unpack copy (layout.hpp): any strided view on either side, e.g.
// a transposed matrix or a (B,H,S,D)->(B,S,H,D) permute. Serves only the
// layouts the 2-D kernels above cannot express.
// ---------------------------------------------------------------------------

// Byte offset of granule `i` (G = 1 << shift bytes each, message order)
// from the view's base. G divides unit and every stride, so a granule never
// straddles a run.
template <class Idx>
__device__ __forceinline__ int64_t nd_offset(const Layout& l, Idx i,
                                             int shift) {
  if (l.ndim == 0) return (int64_t)((uint64_t)i << shift);
  const Idx ug = (Idx)(l.unit >> shift);
  Idx q = i / ug;
  int64_t off = (int64_t)((uint64_t)(i - q * ug) << shift);
#pragma unroll
  for (int d = (int)kMaxDims - 1; d >= 0; --d) {
    if (d < (int)l.ndim) {
      const Idx s = (Idx)l.shape[d];
      const Idx nq = q / s;
      off += (int64_t)(q - nq * s) * l.stride[d];
      q = nq;
    }
  }
  return off;
}

// Generic N-D copy: grid-stride over the message in G-byte granules, in
// message order; each side's address comes from its own layout. Idx is
// uint32_t when the host has checked that the granule count (and so every
// quotient and extent) fits, else uint64_t: 64-bit division costs several
// times the 32-bit one on gfx950 and this kernel does up to 2*(ndim+1) of
// them per granule.
template <int G, class Idx>
__global__ __launch_bounds__(256) void k_copy_nd(
    const uint8_t* __restrict__ src, Layout sl, uint8_t* __restrict__ dst,
    Layout dl, uint64_t n_granules) {
  using V = typename GranuleT<G>::type;
  constexpr int shift = __builtin_ctz(G);
  const Idx n = (Idx)n_granules;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int64_t so = nd_offset<Idx>(sl, (Idx)i, shift);
    const int64_t dof = nd_offset<Idx>(dl, (Idx)i, shift);
    *(V*)(dst + dof) = *(const V*)(src + so);
  }
}

// Transpose family: one side contiguous (dense along the innermost logical
// dimension B), the other a layout of single elements whose unit-stride
// dimension A is not B. A generic copy leaves one side with E-byte accesses
// a whole stride apart; here a workgroup stages a T x T element tile
// through LDS, reading with lanes along the source's dense axis and
// writing with lanes along the destination's. All other dimensions are
// batch dimensions decoded from the tile index.
struct TileArgs {
  uint64_t nA, nB;       // extents of the two tile axes
  int64_t sB;            // strided side: byte stride of B (A's is E)
  uint64_t cA;           // contiguous side: byte stride of A (B's is E)
  uint32_t nbatch;       // batch dimensions, outermost first
  uint32_t s_is_src;     // strided side is the source
  uint64_t bshape[3];
  int64_t bS[3];         // strided side byte strides
  uint64_t bC[3];        // contiguous side byte strides
  uint64_t tilesA, tilesB, tiles;  // tiles = tilesA * tilesB * batch
};

template <int E> struct TileT {
  static constexpr int T = E == 16 ? 32 : 64;
  // Row pad: one access width, and at least one bank (4 B) because sub-
  // dword accesses still bank by dword. Row pitches 68/132/260/520/528 B
  // put the lanes of the transposed phase on distinct banks.
  static constexpr int PAD = E < 4 ? 4 : E;
  static constexpr int PITCH = T * E + PAD;
};

template <int E>
__global__ __launch_bounds__(256) void k_copy_nd_tile(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, TileArgs a) {
  using V = typename GranuleT<E>::type;
  constexpr int T = TileT<E>::T;
  constexpr int PITCH = TileT<E>::PITCH;
  constexpr int ROWS = 256 / T;  // tile rows covered per pass
  __shared__ __attribute__((aligned(16))) uint8_t tile[T * PITCH];
  const int lane = threadIdx.x % T;
  const int row0 = threadIdx.x / T;
  for (uint64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    uint64_t q = t / a.tilesB;
    const uint64_t b0 = (t - q * a.tilesB) * T;
    uint64_t bq = q / a.tilesA;
    const uint64_t a0 = (q - bq * a.tilesA) * T;
    int64_t offS = 0;
    uint64_t offC = 0;
    for (int d = (int)a.nbatch - 1; d >= 0; --d) {
      const uint64_t nq = bq / a.bshape[d];
      const uint64_t idx = bq - nq * a.bshape[d];
      offS += (int64_t)idx * a.bS[d];
      offC += idx * a.bC[d];
      bq = nq;
    }
    // Element (ia, ib) of the tile: strided side at offS + ia*E + ib*sB,
    // contiguous side at offC + ia*cA + ib*E.
    if (a.s_is_src) {
      // Read with lanes along A; LDS is [ib][ia].
      const uint64_t ia = a0 + lane;
      for (int r = row0; r < T; r += ROWS) {
        const uint64_t ib = b0 + r;
        if (ia < a.nA && ib < a.nB)
          *(V*)(tile + r * PITCH + lane * E) =
              *(const V*)(src + offS + (int64_t)(ia * E) + (int64_t)ib * a.sB);
      }
      __syncthreads();
      // Write with lanes along B.
      const uint64_t ob = b0 + lane;
      for (int r = row0; r < T; r += ROWS) {
        const uint64_t oa = a0 + r;
        if (oa < a.nA && ob < a.nB)
          *(V*)(dst + offC + oa * a.cA + ob * E) =
              *(const V*)(tile + lane * PITCH + r * E);
      }
    } else {
      // Read with lanes along B; LDS is [ia][ib].
      const uint64_t ib = b0 + lane;
      for (int r = row0; r < T; r += ROWS) {
        const uint64_t ia = a0 + r;
        if (ia < a.nA && ib < a.nB)
          *(V*)(tile + r * PITCH + lane * E) =
              *(const V*)(src + offC + ia * a.cA + ib * E);
      }
      __syncthreads();
      // Write with lanes along A.
      const uint64_t oa = a0 + lane;
      for (int r = row0; r < T; r += ROWS) {
        const uint64_t ob = b0 + r;
        if (oa < a.nA && ob < a.nB)
          *(V*)(dst + offS + (int64_t)(oa * E) + (int64_t)ob * a.sB) =
              *(const V*)(tile + lane * PITCH + r * E);
      }
    }
    __syncthreads();  // the next tile overwrites the LDS
  }
}

int copy_nd_tile_extent(int elem_bytes) {
  switch (elem_bytes) {
    case 1: return TileT<1>::T;
    case 2: return TileT<2>::T;
    case 4: return TileT<4>::T;
    case 8: return TileT<8>::T;
    case 16: return TileT<16>::T;
  }
  return 0;
}

// Which side is the transposed one, and along which dimension; false when
// the pair is not in the transpose family or an access would be misaligned.
static bool tile_plan(const Layout& sl, const Layout& dl, const void* src,
                      const void* dst, bool* s_is_src, int* axis) {
  const Layout* s = nullptr;
  if (sl.ndim == 0 && dl.ndim >= 2) {
    s = &dl;
    *s_is_src = false;
  } else if (dl.ndim == 0 && sl.ndim >= 2) {
    s = &sl;
    *s_is_src = true;
  } else {
    return false;
  }
  *axis = tile_axis(*s);
  if (*axis < 0) return false;
  return granule(sl, dl, (uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst) >=
         s->unit;
}

bool copy_nd_tile_eligible(const Layout& sl, const Layout& dl, const void* src,
                           const void* dst) {
  bool s_is_src;
  int axis;
  return tile_plan(sl, dl, src, dst, &s_is_src, &axis);
}

// Dispatch rule for CopyNdPath::Auto: the tiled kernel whenever the pair is
// in the transpose family (tile_plan), i.e. the strided side's dense run is
// a single element (<= 16 B), and dimension A fills at least half a tile
// row; the generic kernel for everything else.
//
// Measured on MI355X, fp16, payload GB/s, median of 7 rounds x 10 calls,
// two runs within 1 % of each other, rounds within 7 %
// (docs/benchmark.md "N-D layouts", profiles/nd_layouts_run*.txt):
//   2-D transpose        generic   tiled   .contiguous()+flat   flat
//     64 MiB                 466    1288          391           1810
//     256 MiB                187    1121          431           2373
//   (B,H,S,D)->(B,S,H,D), D=128: 256 B dense runs, not in the family
//     64 MiB                1967       -          837           1834
//     256 MiB               2271       -         1072           2273
// With 256 B runs the generic kernel already matches the flat copy, so
// there is nothing for a tiled kernel to win above single elements. The
// half-row floor is reasoning, not measurement: with fewer elements along A
// most lanes of the phase that runs along A idle, while the generic
// kernel's message-order walk keeps the contiguous side coalesced.
hipError_t launch_copy_nd(void* dst, const Layout& dl, const void* src,
                          const Layout& sl, uint64_t bytes,
                          hipStream_t stream, const CopyTuning& t,
                          CopyNdPath path, IndexWidth width) {
  if (bytes == 0) return hipSuccess;
  bool s_is_src = false;
  int axis = -1;
  const bool eligible = tile_plan(sl, dl, src, dst, &s_is_src, &axis);
  if (path == CopyNdPath::Tiled && !eligible) return hipErrorInvalidValue;
  const size_t cap = t.block_cap;
  const uint8_t* sp = (const uint8_t*)src;
  uint8_t* dp = (uint8_t*)dst;
  if (eligible && path != CopyNdPath::Generic) {
    const Layout& s = s_is_src ? sl : dl;
    const int E = (int)s.unit;
    const int T = copy_nd_tile_extent(E);
    const int B = (int)s.ndim - 1;
    if (path == CopyNdPath::Tiled || s.shape[axis] >= (uint64_t)T / 2) {
      TileArgs a{};
      a.nA = s.shape[axis];
      a.nB = s.shape[B];
      a.sB = s.stride[B];
      a.s_is_src = s_is_src;
      // Contiguous-side strides: row-major over the strided side's own
      // dimensions, which is the message order.
      uint64_t cstride[kMaxDims];
      uint64_t run = (uint64_t)E;
      for (int d = B; d >= 0; --d) {
        cstride[d] = run;
        run *= s.shape[d];
      }
      a.cA = cstride[axis];
      uint64_t batch = 1;
      for (int d = 0; d < B; d++) {
        if (d == axis) continue;
        a.bshape[a.nbatch] = s.shape[d];
        a.bS[a.nbatch] = s.stride[d];
        a.bC[a.nbatch] = cstride[d];
        a.nbatch++;
        batch *= s.shape[d];
      }
      a.tilesA = (a.nA + T - 1) / T;
      a.tilesB = (a.nB + T - 1) / T;
      a.tiles = a.tilesA * a.tilesB * batch;
      const unsigned blocks =
          (unsigned)(a.tiles < cap ? (size_t)a.tiles : cap);
      // tile_plan admits single elements of 1/2/4/8/16 bytes only.
      with_granule((uint64_t)E, [&](auto e) {
        hipLaunchKernelGGL(k_copy_nd_tile<e()>, dim3(blocks), dim3(256), 0,
                           stream, sp, dp, a);
      });
      return hipGetLastError();
    }
  }
  with_granule(
      granule(sl, dl, (uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst),
      [&](auto g) {
        const uint64_t n = bytes / g();
        const dim3 grid(copy_grid(n / 4 + 1, cap));
        // 32-bit index arithmetic only where every value fits: the granule
        // count bounds each quotient and (the message being non-empty) each
        // extent.
        with_index_width(n, width, [&](auto idx) {
          hipLaunchKernelGGL((k_copy_nd<g(), decltype(idx)>), grid, dim3(256),
                             0, stream, sp, sl, dp, dl, n);
        });
      });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Indexed copy (index.hpp): slices of a pool picked by an index list, on
// either side or both, e.g. the scattered blocks of a paged KV cache. A side
// with a null list is one dense run.
//
// The shape of k_copy_strided<16> with a table lookup in place of the row
// multiply: grid-stride over the message in G-byte granules, in message
// order, so consecutive lanes take consecutive granules and accesses inside
// a slice stay coalesced; x4 unroll, no LDS (nothing is reused). Per side
// and granule one division by the slice length and one 4-byte table load;
// the lanes of a wave mostly share the quotient, so the load is served as a
// broadcast out of L1. Both slice sizes are free and independent: slice
// boundaries of the two sides may interleave.
//
// Idx is uint32_t when the host has checked that the granule count (which
// bounds every quotient and both slice lengths) fits, else uint64_t, as in
// k_copy_nd. The byte offset idx * stride is 64-bit either way.
// ---------------------------------------------------------------------------

template <class Idx>
__device__ __forceinline__ uint64_t indexed_offset(const IndexSide& s, Idx g,
                                                   Idx slice_g, int shift) {
  if (s.index == nullptr) return (uint64_t)g << shift;
  const Idx q = g / slice_g;
  return (uint64_t)s.index[q] * s.stride + ((uint64_t)(g - q * slice_g) << shift);
}

template <int G, class Idx>
__global__ __launch_bounds__(256) void k_copy_indexed(
    const uint8_t* __restrict__ src, IndexSide ss, uint8_t* __restrict__ dst,
    IndexSide ds, uint64_t n_granules) {
  using V = typename GranuleT<G>::type;
  constexpr int shift = __builtin_ctz(G);
  // A dense side's slice length is never divided by.
  const Idx sg = (Idx)(ss.slice_bytes >> shift);
  const Idx dg = (Idx)(ds.slice_bytes >> shift);
  const uint64_t n = n_granules;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // 4 independent granules in flight per thread per iteration.
  while (i + 3 * stride < n) {
    V v[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      v[k] = *(const V*)(src + indexed_offset<Idx>(ss, (Idx)(i + k * stride),
                                                   sg, shift));
#pragma unroll
    for (int k = 0; k < 4; k++)
      *(V*)(dst + indexed_offset<Idx>(ds, (Idx)(i + k * stride), dg, shift)) =
          v[k];
    i += 4 * stride;
  }
  for (; i < n; i += stride)
    *(V*)(dst + indexed_offset<Idx>(ds, (Idx)i, dg, shift)) =
        *(const V*)(src + indexed_offset<Idx>(ss, (Idx)i, sg, shift));
}

hipError_t launch_copy_indexed(void* dst, const IndexSide& ds,
                               const void* src, const IndexSide& ss,
                               uint64_t bytes, hipStream_t stream,
                               const CopyTuning& t, IndexWidth width) {
  if (bytes == 0) return hipSuccess;
  // Two dense sides are launch_copy's; an indexed side has whole, non-empty
  // slices that add up to the message.
  if (ds.index == nullptr && ss.index == nullptr) return hipErrorInvalidValue;
  if ((ds.index && (ds.slice_bytes == 0 || bytes % ds.slice_bytes)) ||
      (ss.index && (ss.slice_bytes == 0 || bytes % ss.slice_bytes)))
    return hipErrorInvalidValue;
  const size_t cap = t.block_cap;
  const uint8_t* sp = (const uint8_t*)src;
  uint8_t* dp = (uint8_t*)dst;
  with_granule(
      index_granule((uint64_t)(uintptr_t)dst, ds, (uint64_t)(uintptr_t)src,
                    ss),
      [&](auto g) {
        const uint64_t n = bytes / g();
        const dim3 grid(copy_grid(n / 4 + 1, cap));
        with_index_width(n, width, [&](auto idx) {
          hipLaunchKernelGGL((k_copy_indexed<g(), decltype(idx)>), grid,
                             dim3(256), 0, stream, sp, ss, dp, ds, n);
        });
      });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Accumulate family (reducing receive): dst[i] = dst[i] + src[i]. Same
// shape as the copy family (256-thread workgroups, 16 B per lane, grid
// stride, x4 unroll, no LDS: nothing is reused), but the destination is
// read as well as written, so a message costs three memory streams.
//
// The 2-byte types widen each element to fp32, add there and round once to
// nearest even: exactly (dst.float() + src.float()).to(dtype). Subnormals
// are kept (the default kernel mode; never build this file with
// flush-to-zero).
// ---------------------------------------------------------------------------

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// One tag per element type: W is the element's storage word. up() / down()
// take one element to fp32 and back (down rounds to nearest even); widen()
// / narrow() do the same for the kPerWord elements packed in one 32-bit
// word of a vector. add() works on one element, add32() on one such word.
struct AccF32 {
  using W = uint32_t;
  static constexpr int kPerWord = 1;
  static __device__ __forceinline__ float up(W w) { return __uint_as_float(w); }
  static __device__ __forceinline__ W down(float f) {
    return __float_as_uint(f);
  }
  static __device__ __forceinline__ void widen(uint32_t w, float* f) {
    f[0] = __uint_as_float(w);
  }
  static __device__ __forceinline__ uint32_t narrow(const float* f) {
    return __float_as_uint(f[0]);
  }
  static __device__ __forceinline__ W add(W d, W s) {
    return __float_as_uint(__uint_as_float(d) + __uint_as_float(s));
  }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    return add(d, s);
  }
};

struct AccI32 {
  using W = uint32_t;
  static __device__ __forceinline__ W add(W d, W s) { return d + s; }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    return d + s;
  }
};

struct AccF16 {
  using W = uint16_t;
  static constexpr int kPerWord = 2;
  static __device__ __forceinline__ float up(W w) {
    return (float)__builtin_bit_cast(_Float16, w);
  }
  static __device__ __forceinline__ W down(float f) {
    return __builtin_bit_cast(W, (_Float16)f);
  }
  static __device__ __forceinline__ void widen(uint32_t w, float* f) {
    const f32x2 v =
        __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2);
    f[0] = v.x;
    f[1] = v.y;
  }
  static __device__ __forceinline__ uint32_t narrow(const float* f) {
    f32x2 v;
    v.x = f[0];
    v.y = f[1];
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  }
  static __device__ __forceinline__ W add(W d, W s) {
    return down(up(d) + up(s));
  }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    float a[2], b[2];
    widen(d, a);
    widen(s, b);
    a[0] += b[0];
    a[1] += b[1];
    return narrow(a);
  }
};

struct AccBF16 {
  using W = uint16_t;
  static constexpr int kPerWord = 2;
  // A bf16 is the top half of an fp32: widening is a shift. The narrowing
  // conversion is the compiler's (v_cvt_pk_bf16_f32 on gfx950).
  static __device__ __forceinline__ float up(W w) {
    return __uint_as_float((uint32_t)w << 16);
  }
  static __device__ __forceinline__ W down(float f) {
    return __builtin_bit_cast(W, (__bf16)f);
  }
  static __device__ __forceinline__ void widen(uint32_t w, float* f) {
    f[0] = __uint_as_float(w << 16);
    f[1] = __uint_as_float(w & 0xffff0000u);
  }
  static __device__ __forceinline__ uint32_t narrow(const float* f) {
    f32x2 v;
    v.x = f[0];
    v.y = f[1];
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
  }
  static __device__ __forceinline__ W add(W d, W s) {
    return down(up(d) + up(s));
  }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    float a[2], b[2];
    widen(d, a);
    widen(s, b);
    a[0] += b[0];
    a[1] += b[1];
    return narrow(a);
  }
};

template <class A>
__device__ __forceinline__ u32x4 accum16(u32x4 d, u32x4 s) {
  u32x4 r;
  r.x = A::add32(d.x, s.x);
  r.y = A::add32(d.y, s.y);
  r.z = A::add32(d.z, s.z);
  r.w = A::add32(d.w, s.w);
  return r;
}

// 16B-vector bulk accumulate (both pointers 16B-aligned). The source load
// is plain, or non-temporal (NT) for a large source, which is read exactly
// once and would otherwise sweep the cache the accumulator's
// read-modify-write lives in. The destination stays plain.
template <class A, bool NT>
__global__ __launch_bounds__(256) void k_accum_b128(
    const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // 4 + 4 independent loads in flight per thread per iteration.
  while (i + 3 * stride < n16) {
    u32x4 s0 = ld16<NT>(&src[i]);
    u32x4 s1 = ld16<NT>(&src[i + stride]);
    u32x4 s2 = ld16<NT>(&src[i + 2 * stride]);
    u32x4 s3 = ld16<NT>(&src[i + 3 * stride]);
    u32x4 d0 = dst[i];
    u32x4 d1 = dst[i + stride];
    u32x4 d2 = dst[i + 2 * stride];
    u32x4 d3 = dst[i + 3 * stride];
    dst[i] = accum16<A>(d0, s0);
    dst[i + stride] = accum16<A>(d1, s1);
    dst[i + 2 * stride] = accum16<A>(d2, s2);
    dst[i + 3 * stride] = accum16<A>(d3, s3);
    i += 4 * stride;
  }
  for (; i < n16; i += stride)
    dst[i] = accum16<A>(dst[i], ld16<NT>(&src[i]));
}

// Element-granularity accumulate: heads, tails and pairs that are not 16B
// co-aligned. Both pointers are element-aligned.
template <class A>
__global__ __launch_bounds__(256) void k_accum_elem(
    const typename A::W* __restrict__ src, typename A::W* __restrict__ dst,
    size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = A::add(dst[i], src[i]);
}

template <class A>
static hipError_t launch_accum_t(void* dst, const void* src, size_t bytes,
                                 hipStream_t stream, const CopyTuning& t) {
  using W = typename A::W;
  const size_t cap = t.block_cap;
  uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
  if ((s & 15) == (d & 15)) {
    // Co-aligned: element head, vector bulk, element tail. 16 is a multiple
    // of the element size, so head and tail are whole elements.
    const auto [head, n16, tail] = split16(s, bytes);
    if (head)
      hipLaunchKernelGGL(k_accum_elem<A>, dim3(1), dim3(64), 0, stream,
                         (const W*)s, (W*)d, head / sizeof(W));
    s += head;
    d += head;
    if (n16) {
      const dim3 grid(copy_grid(n16 / 4 + 1, cap));
      // Non-temporal source loads from accum_nt_threshold, a knob of the
      // accumulate family's own: its crossover lies far above the copy
      // family's nt_threshold (see kAccumNtDefaultThreshold).
      if (bytes - head >= t.accum_nt_threshold)
        hipLaunchKernelGGL((k_accum_b128<A, true>), grid, dim3(256), 0,
                           stream, (const u32x4*)s, (u32x4*)d, n16);
      else
        hipLaunchKernelGGL((k_accum_b128<A, false>), grid, dim3(256), 0,
                           stream, (const u32x4*)s, (u32x4*)d, n16);
    }
    if (tail)
      hipLaunchKernelGGL(k_accum_elem<A>, dim3(1), dim3(64), 0, stream,
                         (const W*)(s + n16 * 16), (W*)(d + n16 * 16),
                         tail / sizeof(W));
  } else {
    const size_t n = bytes / sizeof(W);
    hipLaunchKernelGGL(k_accum_elem<A>, dim3(copy_grid(n / 4 + 1, cap)),
                       dim3(256), 0, stream, (const W*)s, (W*)d, n);
  }
  return hipGetLastError();
}

// dst and src must be aligned to the element size and `bytes` a multiple
// of it (the callers in gpu.cpp guarantee both); src must not overlap dst.
hipError_t launch_accum(void* dst, const void* src, size_t bytes,
                        ElemType dtype, hipStream_t stream,
                        const CopyTuning& t) {
  const size_t es = elem_size(dtype);
  if (es == 0 || bytes % es || ((uintptr_t)dst | (uintptr_t)src) % es)
    return hipErrorInvalidValue;
  if (bytes == 0) return hipSuccess;
  switch (dtype) {
    case ElemType::F32: return launch_accum_t<AccF32>(dst, src, bytes, stream, t);
    case ElemType::I32: return launch_accum_t<AccI32>(dst, src, bytes, stream, t);
    case ElemType::F16: return launch_accum_t<AccF16>(dst, src, bytes, stream, t);
    case ElemType::BF16:
      return launch_accum_t<AccBF16>(dst, src, bytes, stream, t);
    case ElemType::None: break;
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// Convert family (converting receive): the message holds one float type,
// the buffer another. dst[i] = D(src[i]), or with ACC
// dst[i] = D(float(dst[i]) + float(src[i])): every element goes through
// fp32 and is rounded once, to nearest even; widening is exact. Exactly
// msg.to(dtype) and (dst.float() + msg.float()).to(dtype). Subnormals are
// kept, as in the accumulate family.
//
// Same shape as that family: 256-thread workgroups, grid stride, x4 unroll,
// no LDS (nothing is reused). A lane takes E consecutive elements, whose
// two sides differ in bytes for a 2-byte <-> 4-byte pair:
//   E = 8 (shape A)  16 B on the narrow side, two adjacent 16 B accesses
//                    on the wide side (a wave instruction then touches
//                    every other 16 B of a 2 KiB window);
//   E = 4 (shape B)  8 B on the narrow side, 16 B on the wide side, both
//                    perfectly lane-contiguous.
// fp16 <-> bf16 is 16 B to 16 B (E = 8) whatever the shape. Which of A and
// B production runs, and the numbers behind it: kConvertProdShape.
//
// Source loads are plain. Whether non-temporal source loads pay off for
// this byte ratio was not measured (the accumulate family's 192 MiB
// crossover was measured for equal widths and does not carry over), so
// there is no non-temporal variant and no threshold.
// ---------------------------------------------------------------------------

// NW 32-bit words at p: one 8 B access, or NW / 4 adjacent 16 B ones. p is
// aligned to min(16, 4 * NW).
template <int NW>
__device__ __forceinline__ void ld_words(const uint8_t* p, uint32_t* w) {
  if constexpr (NW == 2) {
    const uint2 v = *(const uint2*)p;
    w[0] = v.x;
    w[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < NW / 4; q++) {
      const u32x4 v = *(const u32x4*)(p + 16 * q);
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
  }
}
template <int NW>
__device__ __forceinline__ void st_words(const uint32_t* w, uint8_t* p) {
  if constexpr (NW == 2) {
    uint2 v;
    v.x = w[0];
    v.y = w[1];
    *(uint2*)p = v;
  } else {
#pragma unroll
    for (int q = 0; q < NW / 4; q++) {
      u32x4 v;
      v.x = w[4 * q];
      v.y = w[4 * q + 1];
      v.z = w[4 * q + 2];
      v.w = w[4 * q + 3];
      *(u32x4*)(p + 16 * q) = v;
    }
  }
}

// E elements of one lane: source words s, destination words d (read when
// ACC, written always).
template <class S, class D, bool ACC, int E>
__device__ __forceinline__ void convert_lane(const uint32_t* s, uint32_t* d) {
  float f[E];
#pragma unroll
  for (int j = 0; j < E / S::kPerWord; j++)
    S::widen(s[j], &f[j * S::kPerWord]);
  if constexpr (ACC) {
    float g[E];
#pragma unroll
    for (int j = 0; j < E / D::kPerWord; j++)
      D::widen(d[j], &g[j * D::kPerWord]);
#pragma unroll
    for (int e = 0; e < E; e++) f[e] = g[e] + f[e];
  }
#pragma unroll
  for (int j = 0; j < E / D::kPerWord; j++)
    d[j] = D::narrow(&f[j * D::kPerWord]);
}

// Vector bulk: nvec lanes' worth of E elements each. src is aligned to
// min(16, E * sizeof(S::W)), dst to min(16, E * sizeof(D::W)). Offsets are
// 64-bit: a message past 4 Gi elements addresses correctly.
template <class S, class D, bool ACC, int E>
__global__ __launch_bounds__(256) void k_convert_vec(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t nvec) {
  constexpr int SWN = E / S::kPerWord, DWN = E / D::kPerWord;
  constexpr size_t SB = 4 * SWN, DB = 4 * DWN;  // bytes per lane, each side
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // 4 (+ 4 when accumulating) independent loads in flight per thread.
  while (i + 3 * stride < nvec) {
    uint32_t s[4][SWN], d[4][DWN];
#pragma unroll
    for (int k = 0; k < 4; k++) ld_words<SWN>(src + (i + k * stride) * SB, s[k]);
    if constexpr (ACC) {
#pragma unroll
      for (int k = 0; k < 4; k++)
        ld_words<DWN>(dst + (i + k * stride) * DB, d[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      convert_lane<S, D, ACC, E>(s[k], d[k]);
      st_words<DWN>(d[k], dst + (i + k * stride) * DB);
    }
    i += 4 * stride;
  }
  for (; i < nvec; i += stride) {
    uint32_t s[SWN], d[DWN];
    ld_words<SWN>(src + i * SB, s);
    if constexpr (ACC) ld_words<DWN>(dst + i * DB, d);
    convert_lane<S, D, ACC, E>(s, d);
    st_words<DWN>(d, dst + i * DB);
  }
}

// Element granularity: heads, tails and pairs no head can co-align. Both
// pointers are aligned to their own element size.
template <class S, class D, bool ACC>
__global__ __launch_bounds__(256) void k_convert_elem(
    const typename S::W* __restrict__ src, typename D::W* __restrict__ dst,
    size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float f = S::up(src[i]);
    if constexpr (ACC) f = D::up(dst[i]) + f;
    dst[i] = D::down(f);
  }
}

// The lane shape production runs for a 2-byte <-> 4-byte pair: A. Measured
// on MI355X, same-device loopback through the engine, both shapes
// alternated in one process, us per receive, median of 9 rounds x 10 calls
// (min-max over the rounds), two runs (docs/benchmark.md "Converting
// receive", profiles/convert_bench_run*.jsonl); run 1:
//   bf16 message += into fp32      shape A               shape B
//     16 MiB                  48.4 (47.3-56.1)      45.4 (44.2-48.2)
//     64 MiB                  84.5 (82.1-85.4)      82.8 (80.0-84.6)
//     256 MiB                293.3 (289.8-296.5)   341.5 (335.4-347.3)
//   fp32 message into bf16
//     16 MiB                  36.3 (34.3-37.7)      36.0 (34.9-38.2)
//     64 MiB                  47.7 (46.8-49.3)      48.1 (46.0-50.0)
//     256 MiB                107.1 (103.3-109.7)   117.4 (114.3-122.5)
// At 16 and 64 MiB the two are level (ranges overlap; B is ahead by 2-6 %
// in the median for bf16 into fp32); at 256 MiB A takes 14 % and 9 % less
// time with the ranges apart (16 % and 7 % in run 2). B stays built behind
// ConvertShape::B (hooks only).
constexpr ConvertShape kConvertProdShape = ConvertShape::A;

// What ConvertShape::Default resolves to. Production never changes it; the
// bench hook does, so one process can time both shapes through the engine.
static std::atomic<ConvertShape> g_convert_shape{kConvertProdShape};

ConvertShape convert_default_shape() {
  return g_convert_shape.load(std::memory_order_relaxed);
}
void set_convert_default_shape(ConvertShape shape) {
  g_convert_shape.store(
      shape == ConvertShape::Default ? kConvertProdShape : shape,
      std::memory_order_relaxed);
}

static int convert_lane_elems(ElemType dst_type, ElemType src_type,
                              ConvertShape shape) {
  if (shape == ConvertShape::Default) shape = convert_default_shape();
  const bool mixed = elem_size(dst_type) != elem_size(src_type);
  return mixed && shape == ConvertShape::B ? 4 : 8;
}

// Head of h elements, then whole lanes, then a tail. A lane's source access
// is As = min(16, E * ss) bytes wide and its destination access
// Ad = min(16, E * ds), so the bulk may start at element h only if
//   (src + h * ss) % As == 0  and  (dst + h * ds) % Ad == 0.
// Each side repeats with a period of As / ss and Ad / ds elements, both
// powers of two. Solvable iff the two sides' element offsets from their own
// boundary agree modulo the smaller period:
//   (src / ss) % p == (dst / ds) % p,  p = min(As / ss, Ad / ds);
// h is then the smallest solution, below the larger period (at most 7).
// Otherwise the element kernel takes everything.
ConvertPlan convert_plan(uintptr_t dst, ElemType dst_type, uintptr_t src,
                         ElemType src_type, size_t n, ConvertShape shape) {
  const size_t ss = elem_size(src_type), ds = elem_size(dst_type);
  const size_t E = (size_t)convert_lane_elems(dst_type, src_type, shape);
  const size_t as = E * ss < 16 ? E * ss : 16, ad = E * ds < 16 ? E * ds : 16;
  const size_t ps = as / ss, pd = ad / ds;
  ConvertPlan p{};
  p.lane_elems = (int)E;
  for (size_t h = 0; h < (ps > pd ? ps : pd); h++) {
    if ((src + h * ss) % as || (dst + h * ds) % ad) continue;
    p.head = h < n ? h : n;
    p.vectors = (n - p.head) / E;
    p.tail = (n - p.head) % E;
    return p;
  }
  p.elem_only = true;
  p.tail = n;
  return p;
}

template <class S, class D>
static hipError_t launch_convert_t(void* dst, const void* src, size_t n,
                                   bool accumulate, const ConvertPlan& p,
                                   hipStream_t stream, size_t cap) {
  using SW = typename S::W;
  using DW = typename D::W;
  const SW* s = (const SW*)src;
  DW* d = (DW*)dst;
  auto elem = [&](const SW* es, DW* ed, size_t en, dim3 grid, dim3 block) {
    if (accumulate)
      hipLaunchKernelGGL((k_convert_elem<S, D, true>), grid, block, 0, stream,
                         es, ed, en);
    else
      hipLaunchKernelGGL((k_convert_elem<S, D, false>), grid, block, 0,
                         stream, es, ed, en);
  };
  if (p.elem_only) {
    elem(s, d, n, dim3(copy_grid(n / 4 + 1, cap)), dim3(256));
    return hipGetLastError();
  }
  if (p.head) elem(s, d, p.head, dim3(1), dim3(64));
  s += p.head;
  d += p.head;
  if (p.vectors) {
    const dim3 grid(copy_grid(p.vectors / 4 + 1, cap));
    const uint8_t* sb = (const uint8_t*)s;
    uint8_t* db = (uint8_t*)d;
    auto vec = [&](auto e) {
      constexpr int E = decltype(e)::value;
      if (accumulate)
        hipLaunchKernelGGL((k_convert_vec<S, D, true, E>), grid, dim3(256), 0,
                           stream, sb, db, p.vectors);
      else
        hipLaunchKernelGGL((k_convert_vec<S, D, false, E>), grid, dim3(256), 0,
                           stream, sb, db, p.vectors);
    };
    if constexpr (sizeof(SW) != sizeof(DW)) {
      if (p.lane_elems == 4) vec(std::integral_constant<int, 4>{});
      else vec(std::integral_constant<int, 8>{});
    } else {
      vec(std::integral_constant<int, 8>{});
    }
  }
  if (p.tail)
    elem(s + p.vectors * p.lane_elems, d + p.vectors * p.lane_elems, p.tail,
         dim3(1), dim3(64));
  return hipGetLastError();
}

// f(tag) for one of the three float types; false for anything else.
template <class F>
static bool with_float_tag(ElemType t, F&& f) {
  switch (t) {
    case ElemType::F32: f(AccF32{}); return true;
    case ElemType::F16: f(AccF16{}); return true;
    case ElemType::BF16: f(AccBF16{}); return true;
    default: return false;
  }
}

// dst and src must each be aligned to their own element size, the two types
// must differ (equal types are launch_copy's and launch_accum's), and src
// must not overlap dst.
hipError_t launch_convert(void* dst, ElemType dst_type, const void* src,
                          ElemType src_type, size_t n_elems, bool accumulate,
                          hipStream_t stream, const CopyTuning& t) {
  hipError_t result = hipErrorInvalidValue;
  const bool known = with_float_tag(dst_type, [&](auto dtag) {
    with_float_tag(src_type, [&](auto stag) {
      using D = decltype(dtag);
      using S = decltype(stag);
      if constexpr (!std::is_same_v<S, D>) {
        if ((uintptr_t)dst % sizeof(typename D::W) ||
            (uintptr_t)src % sizeof(typename S::W))
          return;
        if (n_elems == 0) {
          result = hipSuccess;
          return;
        }
        const ConvertPlan p =
            convert_plan((uintptr_t)dst, dst_type, (uintptr_t)src, src_type,
                         n_elems, t.convert_shape);
        result = launch_convert_t<S, D>(dst, src, n_elems, accumulate, p,
                                        stream, t.block_cap);
      }
    });
  });
  return known ? result : hipErrorInvalidValue;
}

}  // namespace sw
