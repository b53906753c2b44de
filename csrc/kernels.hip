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

// One tag per element type: W is the element's storage word, add() works
// on one element, add32() on the 32-bit word of a 16 B vector.
struct AccF32 {
  using W = uint32_t;
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
  static __device__ __forceinline__ W add(W d, W s) {
    const float r = (float)__builtin_bit_cast(_Float16, d) +
                    (float)__builtin_bit_cast(_Float16, s);
    return __builtin_bit_cast(W, (_Float16)r);
  }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    const f32x2 r =
        __builtin_convertvector(__builtin_bit_cast(f16x2, d), f32x2) +
        __builtin_convertvector(__builtin_bit_cast(f16x2, s), f32x2);
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
  }
};

struct AccBF16 {
  using W = uint16_t;
  // A bf16 is the top half of an fp32: widening is a shift. The narrowing
  // conversion is the compiler's (v_cvt_pk_bf16_f32 on gfx950).
  static __device__ __forceinline__ W add(W d, W s) {
    const float r = __uint_as_float((uint32_t)d << 16) +
                    __uint_as_float((uint32_t)s << 16);
    return __builtin_bit_cast(W, (__bf16)r);
  }
  static __device__ __forceinline__ uint32_t add32(uint32_t d, uint32_t s) {
    f32x2 r;
    r.x = __uint_as_float(d << 16) + __uint_as_float(s << 16);
    r.y = __uint_as_float(d & 0xffff0000u) + __uint_as_float(s & 0xffff0000u);
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
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

}  // namespace sw
