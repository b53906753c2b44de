// N-D buffer layouts for strided device tensors. Host-only C++ (no HIP, no
// pybind11): used by the bindings, the GPU layer, the kernels' host-side
// dispatch and the GPU-less sanitizer build alike.
//
// A message is the bytes of the view in logical row-major element order
// (what torch's t.contiguous() would hold). A Layout maps a message byte
// offset m to a byte offset from the view's base:
//
//   q = m / unit, r = m % unit;
//   peel q through shape[ndim-1] .. shape[0] (innermost first):
//     idx_d = q % shape[d]; q /= shape[d]; off += idx_d * stride[d];
//   off += r.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace sw {

constexpr uint32_t kMaxDims = 5;

// Plain data without padding: travels inside RtsDesc and as a kernel
// argument.
struct Layout {
  uint32_t ndim;  // dimensions OUTSIDE the dense run; 0 => contiguous
  // Byte length of the dense innermost run. For ndim == 0 it is the
  // message size, saturated (see contiguous_layout): only its low four
  // bits are ever read then.
  uint32_t unit;
  uint64_t shape[kMaxDims];
  int64_t stride[kMaxDims];  // bytes
};
static_assert(sizeof(Layout) == 8 + 16 * kMaxDims);

// The contiguous side of an N-D copy, as a Layout. `unit` cannot hold a
// size >= 4 GiB; it keeps size % 16 so granule() still sees what divides
// the message.
inline Layout contiguous_layout(uint64_t size) {
  Layout l{};
  l.unit = size <= UINT32_MAX ? (uint32_t)size
                              : (uint32_t)(0x80000000u | (size & 15));
  return l;
}

// One dense run `unit` bytes long, `rows` of them `stride` bytes apart:
// today's 2-D row-strided buffer, as a Layout.
inline Layout rows_layout(uint64_t rows, uint64_t row_bytes, uint64_t stride) {
  if (row_bytes > UINT32_MAX)
    throw std::invalid_argument(
        "N-D layout limit: a dense run of 4 GiB or more on the 2-D side");
  Layout l{};
  l.ndim = 1;
  l.unit = (uint32_t)row_bytes;
  l.shape[0] = rows;
  l.stride[0] = (int64_t)stride;
  return l;
}

// Total message bytes of a layout with ndim > 0.
inline uint64_t layout_bytes(const Layout& l) {
  uint64_t n = l.unit;
  for (uint32_t d = 0; d < l.ndim; d++) n *= l.shape[d];
  return n;
}

// Normalise (shape, byte strides, itemsize): drop size-1 dimensions, merge
// neighbours where stride[i] == shape[i+1]*stride[i+1], fold the innermost
// dimension into `unit` when its stride equals itemsize (else unit =
// itemsize). Throws std::invalid_argument for a negative stride, for more
// than kMaxDims remaining dimensions and for a dense run >= 4 GiB under a
// strided dimension. A view without elements normalises to ndim 0, unit 0.
inline Layout normalize(const uint64_t* shape, const int64_t* strides,
                        size_t ndim, uint64_t itemsize) {
  if (itemsize == 0) throw std::invalid_argument("itemsize must be positive");
  for (size_t i = 0; i < ndim; i++)
    if (shape[i] == 0) return Layout{};
  // Worst case before merging is bounded only by the caller's rank; merge
  // in place into a small vector-like pair of arrays grown on the stack.
  constexpr size_t kCap = 64;
  if (ndim > kCap)
    throw std::invalid_argument("N-D layout limit: more than 64 dimensions");
  uint64_t sh[kCap];
  int64_t st[kCap];
  size_t n = 0;
  for (size_t i = 0; i < ndim; i++) {
    if (shape[i] == 1) continue;
    if (strides[i] < 0)
      throw std::invalid_argument(
          "N-D layout limit: negative strides are not supported");
    if (n > 0 && st[n - 1] == (int64_t)(shape[i] * (uint64_t)strides[i])) {
      sh[n - 1] *= shape[i];
      st[n - 1] = strides[i];
    } else {
      sh[n] = shape[i];
      st[n] = strides[i];
      n++;
    }
  }
  uint64_t unit = itemsize;
  if (n > 0 && st[n - 1] == (int64_t)itemsize) {
    unit = sh[n - 1] * itemsize;
    n--;
  }
  Layout l{};
  if (n == 0) return contiguous_layout(unit);
  if (n > kMaxDims)
    throw std::invalid_argument(
        "N-D layout limit: " + std::to_string(n) +
        " dimensions remain after merging, at most " +
        std::to_string(kMaxDims) + " are supported");
  if (unit > UINT32_MAX)
    throw std::invalid_argument(
        "N-D layout limit: a dense run of 4 GiB or more inside a strided "
        "view");
  l.ndim = (uint32_t)n;
  l.unit = (uint32_t)unit;
  for (size_t i = 0; i < n; i++) {
    l.shape[i] = sh[i];
    l.stride[i] = st[i];
  }
  return l;
}

// A destination must not write one byte twice. Walking the dimensions from
// the smallest stride up, each stride has to clear the extent (last byte +
// 1) of everything inside it. Throws std::invalid_argument otherwise.
inline void check_no_overlap(const Layout& l) {
  uint32_t order[kMaxDims];
  for (uint32_t i = 0; i < l.ndim; i++) order[i] = i;
  for (uint32_t i = 1; i < l.ndim; i++)  // insertion sort by stride
    for (uint32_t j = i; j > 0 && l.stride[order[j]] < l.stride[order[j - 1]];
         j--) {
      uint32_t t = order[j];
      order[j] = order[j - 1];
      order[j - 1] = t;
    }
  uint64_t extent = l.unit;
  for (uint32_t k = 0; k < l.ndim; k++) {
    uint32_t d = order[k];
    if (l.stride[d] <= 0)
      throw std::invalid_argument(
          "N-D layout limit: destination elements overlap (stride 0 over " +
          std::to_string(l.shape[d]) + " elements)");
    if ((uint64_t)l.stride[d] < extent)
      throw std::invalid_argument(
          "N-D layout limit: destination elements overlap (stride " +
          std::to_string(l.stride[d]) + " B inside an extent of " +
          std::to_string(extent) + " B)");
    extent += (l.shape[d] - 1) * (uint64_t)l.stride[d];
  }
}

// Largest power of two <= 16 dividing both units, every stride of both
// layouts and both base addresses: the widest access every granule of the
// message can be moved with on both sides.
inline uint32_t granule(const Layout& src, const Layout& dst, uint64_t src_ptr,
                        uint64_t dst_ptr) {
  uint64_t bits = src_ptr | dst_ptr | src.unit | dst.unit | 16;
  for (uint32_t d = 0; d < src.ndim; d++) bits |= (uint64_t)src.stride[d];
  for (uint32_t d = 0; d < dst.ndim; d++) bits |= (uint64_t)dst.stride[d];
  return (uint32_t)(bits & (~bits + 1));
}

// Transpose family: `s` has single elements as its dense run (unit ==
// itemsize <= 16, a power of two) and a unit-stride dimension that is not
// the innermost one. Returns that dimension's index, or -1.
inline int tile_axis(const Layout& s) {
  if (s.ndim < 2) return -1;
  if (s.unit > 16 || (s.unit & (s.unit - 1)) != 0 || s.unit == 0) return -1;
  for (uint32_t d = 0; d + 1 < s.ndim; d++)
    if (s.stride[d] == (int64_t)s.unit) return (int)d;
  return -1;
}

}  // namespace sw
