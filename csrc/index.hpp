// Indexed buffers: slices of a pool picked by an index list (pool[idx]).
// Host-only C++ (no HIP, no pybind11), like layout.hpp: used by the
// bindings, the engine, the GPU layer, the kernels' host-side dispatch and
// the GPU-less sanitizer build alike.
//
// A message is the slices pool[idx[0]], pool[idx[1]], ... in that order,
// each `slice_bytes` dense bytes. Message byte m lies at
//
//   base + idx[m / slice_bytes] * stride + m % slice_bytes
//
// with `stride` the byte distance between two neighbouring slices of the
// pool. All of it is 64-bit arithmetic: idx * stride alone may pass 2^32.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace sw {

// Most entries one index list may hold (a 256 KiB table on the wire and on
// the device).
constexpr uint32_t kIndexMax = 65536;

using IndexList = std::vector<uint32_t>;

// The index of a buffer: a shared immutable list (validated and copied when
// the operation is posted) plus the slice geometry. A null list means the
// buffer is not indexed.
struct IndexRef {
  std::shared_ptr<const IndexList> list;
  uint64_t slice_bytes = 0;
  uint64_t stride = 0;
  bool on() const { return list != nullptr; }
  uint64_t count() const { return list ? list->size() : 0; }
};

// One side of an indexed copy as the kernel sees it: a DEVICE copy of the
// list, or null for a side that is one dense run (base + m).
struct IndexSide {
  const uint32_t* index;
  uint64_t slice_bytes;
  uint64_t stride;
};

// Validate `n` candidate entries against a pool of `extent` slices and copy
// them. A destination (`writable`) must not name a slice twice: two message
// slices would race for it. Throws std::invalid_argument naming the limit.
inline std::shared_ptr<const IndexList> plan_index(const int64_t* v, size_t n,
                                                   uint64_t extent,
                                                   bool writable) {
  if (extent > UINT32_MAX)
    throw std::invalid_argument(
        "index limit: the buffer's first dimension must be below 2**32");
  if (n > kIndexMax)
    throw std::invalid_argument("index limit: " + std::to_string(n) +
                                " entries, at most " +
                                std::to_string(kIndexMax) +
                                " (kIndexMax) are supported");
  auto list = std::make_shared<IndexList>(n);
  for (size_t i = 0; i < n; i++) {
    if (v[i] < 0)
      throw std::invalid_argument("index limit: entry " + std::to_string(i) +
                                  " is negative (" + std::to_string(v[i]) +
                                  ")");
    if ((uint64_t)v[i] >= extent)
      throw std::invalid_argument(
          "index limit: entry " + std::to_string(i) + " (" +
          std::to_string(v[i]) + ") is out of range for a first dimension of " +
          std::to_string(extent));
    (*list)[i] = (uint32_t)v[i];
  }
  if (writable && n > 1) {
    // This runs when a receive is posted, inside the time to delivery, so
    // it is one linear pass whatever the pool's size: an open-addressed
    // table of at least 2n slots. (Sorting a copy took longer for 16384
    // entries than moving their 256 MiB: docs/benchmark.md "Indexed
    // slices".) Entries are below extent <= 2^32 - 1, so ~0 marks a free
    // slot.
    size_t slots = 16;
    while (slots < 2 * n) slots <<= 1;
    std::vector<uint32_t> table(slots, UINT32_MAX);
    for (uint32_t e : *list) {
      size_t h = ((size_t)e * 2654435761u) & (slots - 1);
      while (table[h] != UINT32_MAX) {
        if (table[h] == e)
          throw std::invalid_argument(
              "index limit: a destination index must not repeat an entry (" +
              std::to_string(e) + " appears twice)");
        h = (h + 1) & (slots - 1);
      }
      table[h] = e;
    }
  }
  return list;
}

// Byte offset from the buffer's base of message byte `m`.
inline uint64_t index_offset(const IndexList& list, uint64_t slice_bytes,
                             uint64_t stride, uint64_t m) {
  if (slice_bytes == 0 || m / slice_bytes >= list.size())
    throw std::invalid_argument("index_offset: message offset " +
                                std::to_string(m) + " is outside the message");
  return (uint64_t)list[m / slice_bytes] * stride + m % slice_bytes;
}

// Largest power of two <= 16 dividing both base addresses and, of every
// indexed side, the slice size and the stride: the widest access every
// granule of the message can be moved with on both sides (the granule()
// rule of layout.hpp). A dense side adds nothing: its offsets are the
// message offsets, which the other side's slice size already divides.
inline uint32_t index_granule(uint64_t dst_ptr, const IndexSide& dst,
                              uint64_t src_ptr, const IndexSide& src) {
  uint64_t bits = dst_ptr | src_ptr | 16;
  if (dst.index) bits |= dst.slice_bytes | dst.stride;
  if (src.index) bits |= src.slice_bytes | src.stride;
  return (uint32_t)(bits & (~bits + 1));
}

// ---------------------------------------------------------------------------
// Wire: the FT_RTS_INDEXED payload is an unchanged RtsDesc for the pool's
// base (opaque here, `desc_len` bytes), then IndexWire, then `count` u32
// entries.
// ---------------------------------------------------------------------------

#pragma pack(push, 1)
struct IndexWire {
  uint64_t slice_bytes;
  uint64_t stride;
  uint32_t count;
  uint32_t pad;
};
#pragma pack(pop)
static_assert(sizeof(IndexWire) == 24);

inline std::vector<uint8_t> encode_rts_indexed(const void* desc,
                                               size_t desc_len,
                                               const IndexRef& ix) {
  IndexWire w{ix.slice_bytes, ix.stride, (uint32_t)ix.count(), 0};
  const size_t table = (size_t)w.count * sizeof(uint32_t);
  std::vector<uint8_t> out(desc_len + sizeof(w) + table);
  memcpy(out.data(), desc, desc_len);
  memcpy(out.data() + desc_len, &w, sizeof(w));
  if (table) memcpy(out.data() + desc_len + sizeof(w), ix.list->data(), table);
  return out;
}

// Decode the part after the descriptor of a payload announcing `size`
// message bytes. The payload comes from the peer, so it is refused unless
// its length agrees with its count, the count is within kIndexMax and the
// slices multiply out to exactly `size`.
inline bool decode_rts_indexed(const uint8_t* payload, size_t len,
                               size_t desc_len, uint64_t size, IndexRef* out,
                               std::string* err) {
  if (len < desc_len + sizeof(IndexWire)) {
    *err = "indexed RTS: payload shorter than its header";
    return false;
  }
  IndexWire w;
  memcpy(&w, payload + desc_len, sizeof(w));
  if (w.count > kIndexMax) {
    *err = "indexed RTS: more than kIndexMax entries";
    return false;
  }
  if (len != desc_len + sizeof(w) + (size_t)w.count * sizeof(uint32_t)) {
    *err = "indexed RTS: payload length disagrees with its entry count";
    return false;
  }
  if (w.count > 0 && w.slice_bytes == 0) {
    *err = "indexed RTS: empty slices";
    return false;
  }
  // count * slice_bytes == size, without letting the product wrap.
  if (w.count == 0 ? size != 0
                   : (size % w.count != 0 || size / w.count != w.slice_bytes)) {
    *err = "indexed RTS: slices do not add up to the message size";
    return false;
  }
  auto list = std::make_shared<IndexList>(w.count);
  if (w.count)
    memcpy(list->data(), payload + desc_len + sizeof(w),
           (size_t)w.count * sizeof(uint32_t));
  out->list = std::move(list);
  out->slice_bytes = w.slice_bytes;
  out->stride = w.stride;
  return true;
}

}  // namespace sw
