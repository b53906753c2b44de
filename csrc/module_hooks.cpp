// starway_amd._core — test and bench hooks: every `_`-prefixed function,
// class and constant of the module. None is public API; the engine calls
// none of what they call (gpu_hooks.hpp).
#include "buffer_parse.hpp"
#include "copy_stream.hpp"
#include "gpu_hooks.hpp"

#include <pybind11/stl.h>

namespace sw {
namespace {

// Run fn(args..., &err) with the GIL released. A false (or null) result
// raises RuntimeError("<what>: <err>"); anything else is handed back.
template <class Fn, class... Args>
auto released(const char* what, Fn fn, Args&&... args) {
  std::string err;
  auto r = [&] {
    py::gil_scoped_release rel;
    return fn(std::forward<Args>(args)..., &err);
  }();
  if (!r) throw std::runtime_error(std::string(what) + ": " + err);
  return r;
}

CopyNdPath parse_copy_nd_path(const std::string& path) {
  if (path == "auto") return CopyNdPath::Auto;
  if (path == "generic") return CopyNdPath::Generic;
  if (path == "tiled") return CopyNdPath::Tiled;
  throw py::value_error("copy_nd_sync: path must be auto, generic or tiled");
}

// wide_index of _copy_nd_sync and _copy_index_sync: the 64-bit index
// kernels on a message of any size.
IndexWidth index_width(bool wide) {
  return wide ? IndexWidth::Wide : IndexWidth::Auto;
}

// shape of _convert_sync / _convert_plan / _convert_shape.
ConvertShape parse_convert_shape(const char* what, const std::string& shape) {
  if (shape.empty()) return ConvertShape::Default;
  if (shape == "a") return ConvertShape::A;
  if (shape == "b") return ConvertShape::B;
  throw py::value_error(std::string(what) + ": shape must be 'a', 'b' or ''");
}

// (destination, source) types of the convert hooks: two different ones of
// float32, float16, bfloat16.
std::pair<ElemType, ElemType> convert_pair(const char* what,
                                           const std::string& dst_dtype,
                                           const std::string& src_dtype) {
  const ElemType dt = parse_elem_type(dst_dtype);
  const ElemType st = parse_elem_type(src_dtype);
  for (const auto& [t, name] : {std::pair{dt, dst_dtype}, {st, src_dtype}})
    if (t != ElemType::F32 && t != ElemType::F16 && t != ElemType::BF16)
      throw py::value_error(std::string(what) + ": unsupported dtype '" +
                            name + "'");
  if (dt == st)
    throw py::value_error(std::string(what) + ": the two dtypes are equal "
                          "(that is _copy_device_sync's or _accum_sync's)");
  return {dt, st};
}

// One side of _copy_index_sync: None for a dense side.
IndexRef hook_index_side(py::object index, uint64_t slice_bytes,
                         uint64_t stride, bool writable) {
  IndexRef r;
  if (index.is_none()) return r;
  if (slice_bytes == 0 || (writable && stride < slice_bytes))
    throw py::value_error(std::string("copy_index_sync: bad ") +
                          (writable ? "destination" : "source") +
                          " slice size or stride");
  std::vector<int64_t> v = index.cast<std::vector<int64_t>>();
  r.list = plan_index(v.data(), v.size(), (uint64_t)UINT32_MAX, writable);
  r.slice_bytes = slice_bytes;
  r.stride = stride;
  return r;
}

// (unit, [(extent, stride_bytes), ...]): a Layout as the test hooks see it.
using Plan = std::pair<uint64_t, std::vector<std::pair<uint64_t, int64_t>>>;

Plan plan_of(const Layout& l) {
  Plan p;
  p.first = l.unit;
  for (uint32_t d = 0; d < l.ndim; d++)
    p.second.emplace_back(l.shape[d], l.stride[d]);
  return p;
}

Layout layout_of(const Plan& p) {
  if (p.second.size() > kMaxDims)
    throw std::invalid_argument("N-D layout limit: too many dimensions");
  if (p.first > UINT32_MAX)
    throw std::invalid_argument("N-D layout limit: unit of 4 GiB or more");
  Layout l{};
  l.ndim = (uint32_t)p.second.size();
  l.unit = (uint32_t)p.first;
  for (uint32_t d = 0; d < l.ndim; d++) {
    l.shape[d] = p.second[d].first;
    l.stride[d] = p.second[d].second;
  }
  return l;
}

Layout layout_from(const std::vector<uint64_t>& shape,
                   const std::vector<int64_t>& strides, uint64_t itemsize,
                   bool writable) {
  if (shape.size() != strides.size())
    throw std::invalid_argument("shape and strides differ in length");
  Layout l = normalize(shape.data(), strides.data(), shape.size(), itemsize);
  if (writable) check_no_overlap(l);
  return l;
}

// Inbox test hooks: a ring is either live (device memory from
// inbox_create) or detached (geometry only, built from Python: it lets the
// argument checks run without a device and is refused by everything that
// would touch one).
struct PyInboxRing {
  gpu::InboxInfo info;
  bool live = false;
  uint32_t payload_max() const {
    return info.slot_bytes - gpu::kInboxHdrBytes;
  }
};

struct PyArmTicket {
  void* ticket = nullptr;
};

void need_live(const PyInboxRing& r, const char* what) {
  if (!r.live)
    throw std::runtime_error(std::string(what) +
                             ": ring has no device memory (detached or "
                             "destroyed)");
}

void need_ticket(const PyArmTicket& t, const char* what) {
  if (!t.ticket)
    throw std::runtime_error(std::string(what) + ": ticket already ended");
}

void check_inbox_batch(const char* what, size_t n) {
  if (n < 1 || n > 32)
    throw py::value_error(std::string(what) + ": need 1..32 descriptors");
}

void check_inbox_msg(const char* what, const PyInboxRing& r, uint64_t seq,
                     uint64_t size) {
  if (seq == 0)
    throw py::value_error(std::string(what) +
                          ": seq 0 is the empty-slot sentinel");
  if (size > r.payload_max())
    throw py::value_error(std::string(what) + ": size " +
                          std::to_string(size) + " exceeds payload_max " +
                          std::to_string(r.payload_max()));
}

}  // namespace

void bind_hooks(py::module_& m) {
  // Test/bench hooks: run the gfx950 copy kernels synchronously on raw
  // device pointers. Tuning arguments of 0 mean the process default
  // (_copy_tuning()); explicit values let one process reach every kernel
  // variant and a capped (multi-iteration) grid at small sizes.
  m.def("_copy_device_sync",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, int device,
           size_t block_cap, size_t nt_threshold, int nt_unroll,
           size_t stream_threshold, size_t stream_blocks) {
          const CopyTuning tuning{.block_cap = block_cap,
                                  .nt_threshold = nt_threshold,
                                  .nt_unroll = nt_unroll,
                                  .stream_threshold = stream_threshold,
                                  .stream_blocks = stream_blocks};
          released("copy_device_sync", gpu::copy_device_sync, (void*)dst,
                   (const void*)src, nbytes, device, tuning);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("device"),
        py::arg("block_cap") = 0, py::arg("nt_threshold") = 0,
        py::arg("nt_unroll") = 0, py::arg("stream_threshold") = 0,
        py::arg("stream_blocks") = 0);
  m.def("_copy_strided_sync",
        [](uintptr_t dst, uint64_t dst_stride, uintptr_t src,
           uint64_t src_stride, uint64_t rows, uint64_t row_bytes, int device,
           size_t block_cap) {
          released("copy_strided_sync", gpu::copy_strided_sync, (void*)dst,
                   dst_stride, (const void*)src, src_stride, rows, row_bytes,
                   device, block_cap);
        },
        py::arg("dst"), py::arg("dst_stride"), py::arg("src"),
        py::arg("src_stride"), py::arg("rows"), py::arg("row_bytes"),
        py::arg("device"), py::arg("block_cap") = 0);
  // The accumulate kernels (reducing receive): dst[i] += src[i] over
  // nbytes / itemsize elements of `dtype` (float32, float16, bfloat16,
  // int32). Synchronous, on the pull stream, like _copy_device_sync.
  // nt_threshold is CopyTuning::accum_nt_threshold, not the copies' knob.
  m.def("_accum_sync",
        [](uintptr_t dst, uintptr_t src, size_t nbytes,
           const std::string& dtype, int device, size_t block_cap,
           size_t nt_threshold) {
          const ElemType et = parse_elem_type(dtype);
          if (et == ElemType::None)
            throw py::value_error("accum_sync: unsupported dtype '" + dtype +
                                  "'");
          if (nbytes % elem_size(et) || (dst | src) % elem_size(et))
            throw py::value_error("accum_sync: pointers and length must be "
                                  "multiples of the item size");
          const CopyTuning tuning{.block_cap = block_cap,
                                  .accum_nt_threshold = nt_threshold};
          released("accum_sync", gpu::accum_sync, (void*)dst,
                   (const void*)src, nbytes, et, device, tuning);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("dtype"),
        py::arg("device"), py::arg("block_cap") = 0,
        py::arg("nt_threshold") = 0);
  // The convert kernels (converting receive): dst[i] = dst_dtype(src[i]),
  // or with accumulate dst_dtype(float(dst[i]) + float(src[i])), over
  // n_elems elements; two different types of float32, float16, bfloat16.
  // shape: "a", "b" or "" (what production runs). The family has no
  // non-temporal variant, so nt_threshold takes 0 only. Everything is
  // checked before a device is touched.
  m.def("_convert_sync",
        [](uintptr_t dst, uintptr_t src, size_t n_elems,
           const std::string& dst_dtype, const std::string& src_dtype,
           int device, bool accumulate, size_t block_cap,
           const std::string& shape, size_t nt_threshold) {
          const auto [dt, st] = convert_pair("convert_sync", dst_dtype,
                                             src_dtype);
          if (dst % elem_size(dt) || src % elem_size(st))
            throw py::value_error("convert_sync: each pointer must be a "
                                  "multiple of its item size");
          if (nt_threshold != 0)
            throw py::value_error("convert_sync: the convert kernels have no "
                                  "non-temporal variant (nt_threshold must "
                                  "be 0)");
          const CopyTuning tuning{
              .block_cap = block_cap,
              .convert_shape = parse_convert_shape("convert_sync", shape)};
          released("convert_sync", gpu::convert_sync, (void*)dst, dt,
                   (const void*)src, st, n_elems, accumulate, device, tuning);
        },
        py::arg("dst"), py::arg("src"), py::arg("n_elems"),
        py::arg("dst_dtype"), py::arg("src_dtype"), py::arg("device"),
        py::kw_only(), py::arg("accumulate") = false,
        py::arg("block_cap") = 0, py::arg("shape") = "",
        py::arg("nt_threshold") = 0);
  // The split launch_convert makes of such a message: kernel "vector"
  // (head, vectors of lane_elems elements, tail) or "element" (no head
  // co-aligns the two sides; tail is everything). Host only.
  m.def("_convert_plan",
        [](uintptr_t dst, uintptr_t src, size_t n_elems,
           const std::string& dst_dtype, const std::string& src_dtype,
           const std::string& shape) {
          const auto [dt, st] = convert_pair("convert_plan", dst_dtype,
                                             src_dtype);
          if (dst % elem_size(dt) || src % elem_size(st))
            throw py::value_error("convert_plan: each pointer must be a "
                                  "multiple of its item size");
          const ConvertPlan p = gpu::convert_plan(
              dst, dt, src, st, n_elems,
              parse_convert_shape("convert_plan", shape));
          py::dict d;
          d["kernel"] = p.elem_only ? "element" : "vector";
          d["lane_elems"] = p.lane_elems;
          d["head"] = p.head;
          d["vectors"] = p.vectors;
          d["tail"] = p.tail;
          return d;
        },
        py::arg("dst"), py::arg("src"), py::arg("n_elems"),
        py::arg("dst_dtype"), py::arg("src_dtype"), py::arg("shape") = "");
  // The lane shape production launches run ("a" or "b"). With an argument,
  // a bench's override of it for this process ("" restores the production
  // shape); returns the shape now in effect. Host only.
  m.def("_convert_shape",
        [](py::object shape) {
          if (!shape.is_none())
            gpu::set_convert_default_shape(parse_convert_shape(
                "convert_shape", shape.cast<std::string>()));
          return gpu::convert_default_shape() == ConvertShape::A ? "a" : "b";
        },
        py::arg("shape") = py::none());
  // descs: list of (dst, src, nbytes); one k_copy_multi launch.
  m.def("_copy_multi_sync",
        [](const std::vector<std::tuple<uintptr_t, uintptr_t, uint64_t>>&
               descs,
           int device) {
          if (descs.empty() || descs.size() > (size_t)kMultiMax)
            throw py::value_error("copy_multi_sync: need 1..8 descriptors");
          gpu::CopyDesc d[kMultiMax];
          for (size_t i = 0; i < descs.size(); i++) {
            auto [dst, src, nbytes] = descs[i];
            if (nbytes >= (1ull << 32))
              throw py::value_error(
                  "copy_multi_sync: descriptor size must be < 2**32");
            d[i] = {(void*)dst, (const void*)src, nbytes};
          }
          released("copy_multi_sync", gpu::copy_multi_sync, d,
                   (int)descs.size(), device);
        },
        py::arg("descs"), py::arg("device"));
  // N-D layouts (layout.hpp). The two _plan_* hooks are host-only and work
  // without a GPU. A plan is (unit, [(extent, stride_bytes), ...]), outermost
  // dimension first; an empty list means contiguous.
  m.def("_plan_layout",
        [](const std::vector<uint64_t>& shape,
           const std::vector<int64_t>& strides, uint64_t itemsize,
           bool writable) {
          return plan_of(layout_from(shape, strides, itemsize, writable));
        },
        py::arg("shape"), py::arg("strides_bytes"), py::arg("itemsize"),
        py::arg("writable") = false);
  m.def("_plan_granule",
        [](const Plan& src, const Plan& dst, uint64_t src_ptr,
           uint64_t dst_ptr) {
          return granule(layout_of(src), layout_of(dst), src_ptr, dst_ptr);
        },
        py::arg("src_plan"), py::arg("dst_plan"), py::arg("src_ptr"),
        py::arg("dst_ptr"));
  m.def("_copy_nd_sync",
        [](uintptr_t dst, const std::vector<uint64_t>& dst_shape,
           const std::vector<int64_t>& dst_strides, uintptr_t src,
           const std::vector<uint64_t>& src_shape,
           const std::vector<int64_t>& src_strides, uint64_t itemsize,
           int device, size_t block_cap, const std::string& path,
           bool wide_index) {
          const CopyNdPath p = parse_copy_nd_path(path);
          const IndexWidth w = index_width(wide_index);
          uint64_t dbytes = itemsize, sbytes = itemsize;
          for (uint64_t e : dst_shape) dbytes *= e;
          for (uint64_t e : src_shape) sbytes *= e;
          if (dbytes != sbytes)
            throw py::value_error("copy_nd_sync: source holds " +
                                  std::to_string(sbytes) +
                                  " B, destination " + std::to_string(dbytes));
          Layout dl = layout_from(dst_shape, dst_strides, itemsize, true);
          Layout sl = layout_from(src_shape, src_strides, itemsize, false);
          released("copy_nd_sync", [&](std::string* err) {
            bool ineligible = false;
            const bool ok = gpu::copy_nd_sync((void*)dst, dl, (const void*)src,
                                              sl, sbytes, device, block_cap, p,
                                              w, &ineligible, err);
            // Thrown with the GIL released: a plain C++ exception until
            // pybind11 translates it, by when the GIL is held again.
            if (ineligible) throw py::value_error("copy_nd_sync: " + *err);
            return ok;
          });
        },
        py::arg("dst"), py::arg("dst_shape"), py::arg("dst_strides"),
        py::arg("src"), py::arg("src_shape"), py::arg("src_strides"),
        py::arg("itemsize"), py::arg("device"), py::arg("block_cap") = 0,
        py::arg("path") = "auto", py::arg("wide_index") = false);
  // Indexed buffers (index.hpp). _plan_index, _index_offset and the two
  // descriptor hooks are host-only and work without a GPU.
  m.attr("_INDEX_MAX") = kIndexMax;
  m.attr("_RTS_DESC_BYTES") = sizeof(RtsDesc);
  m.attr("_PROTO_VERSION") = kProtoVersion;
  m.attr("_FT_RTS_INDEXED") = (int)FT_RTS_INDEXED;
  m.def("_plan_index",
        [](py::object index, uint64_t extent, bool writable) {
          return *parse_index(std::move(index), extent, writable);
        },
        py::arg("index"), py::arg("extent"), py::arg("writable") = false);
  m.def("_index_offset",
        [](const std::vector<uint32_t>& index, uint64_t slice_bytes,
           uint64_t stride, uint64_t m) {
          return index_offset(index, slice_bytes, stride, m);
        },
        py::arg("index"), py::arg("slice_bytes"), py::arg("stride"),
        py::arg("m"));
  // The FT_RTS_INDEXED payload around an opaque descriptor of
  // _RTS_DESC_BYTES bytes; decode takes the message size the frame header
  // announces and returns (index, slice_bytes, stride) or raises ValueError.
  m.def("_index_desc_encode",
        [](py::bytes desc, const std::vector<uint32_t>& index,
           uint64_t slice_bytes, uint64_t stride) {
          std::string d = desc;
          if (d.size() != sizeof(RtsDesc))
            throw py::value_error("index_desc_encode: descriptor must be "
                                  "_RTS_DESC_BYTES long");
          IndexRef ix;
          ix.list = std::make_shared<const IndexList>(index);
          ix.slice_bytes = slice_bytes;
          ix.stride = stride;
          std::vector<uint8_t> out = encode_rts_indexed(d.data(), d.size(), ix);
          return py::bytes((const char*)out.data(), out.size());
        },
        py::arg("desc"), py::arg("index"), py::arg("slice_bytes"),
        py::arg("stride"));
  m.def("_index_desc_decode",
        [](py::bytes payload, uint64_t size) {
          std::string p = payload;
          IndexRef ix;
          std::string err;
          if (!decode_rts_indexed((const uint8_t*)p.data(), p.size(),
                                  sizeof(RtsDesc), size, &ix, &err))
            throw py::value_error(err);
          return py::make_tuple(*ix.list, ix.slice_bytes, ix.stride);
        },
        py::arg("payload"), py::arg("size"));
  // One k_copy_indexed launch on raw device pointers; None for a dense
  // side. The arguments are checked before any device is touched.
  // wide_index runs the 64-bit index kernel whatever the message size.
  m.def("_copy_index_sync",
        [](uintptr_t dst, py::object dst_index, uint64_t dst_slice,
           uint64_t dst_stride, uintptr_t src, py::object src_index,
           uint64_t src_slice, uint64_t src_stride, uint64_t bytes, int device,
           size_t block_cap, bool wide_index) {
          if (dst_index.is_none() && src_index.is_none())
            throw py::value_error("copy_index_sync: both sides are dense "
                                  "(that is _copy_device_sync's)");
          IndexRef di = hook_index_side(dst_index, dst_slice, dst_stride,
                                        /*writable=*/true);
          IndexRef si = hook_index_side(src_index, src_slice, src_stride,
                                        /*writable=*/false);
          if (di.on() && di.count() * dst_slice != bytes)
            throw py::value_error(
                "copy_index_sync: destination slices hold " +
                std::to_string(di.count() * dst_slice) + " B, message " +
                std::to_string(bytes));
          if (si.on() && si.count() * src_slice != bytes)
            throw py::value_error(
                "copy_index_sync: source slices hold " +
                std::to_string(si.count() * src_slice) + " B, message " +
                std::to_string(bytes));
          released("copy_index_sync", gpu::copy_index_sync, (void*)dst, di,
                   (const void*)src, si, bytes, device, block_cap,
                   index_width(wide_index));
        },
        py::arg("dst"), py::arg("dst_index"), py::arg("dst_slice"),
        py::arg("dst_stride"), py::arg("src"), py::arg("src_index"),
        py::arg("src_slice"), py::arg("src_stride"), py::arg("bytes"),
        py::arg("device"), py::arg("block_cap") = 0,
        py::arg("wide_index") = false);
  // Tile extents of k_copy_nd_tile: element bytes -> (T_A, T_B) elements.
  {
    py::dict tiles;
    for (int e : {1, 2, 4, 8, 16}) {
      int t = gpu::copy_nd_tile_extent(e);
      tiles[py::int_(e)] = py::make_tuple(t, t);
    }
    m.attr("_ND_TILE") = tiles;
    m.attr("_ND_MAX_DIMS") = kMaxDims;
  }
  m.def("_copy_tuning", [] {
    CopyTuning t = gpu::copy_tuning();
    py::dict d;
    d["block_cap"] = t.block_cap;
    d["nt_threshold"] = t.nt_threshold;
    d["nt_unroll"] = t.nt_unroll;
    return d;
  });
  // Streaming-kernel defaults (copy_stream.hpp), kept out of _copy_tuning()
  // so that dict stays exactly its three keys. "unroll" is the production
  // kernel's U: a tile is 256 * unroll elements of 16 B. Host-only.
  m.def("_copy_stream_tuning", [] {
    CopyTuning t = gpu::copy_tuning();
    py::dict d;
    d["stream_threshold"] = t.stream_threshold;
    d["stream_blocks"] = t.stream_blocks;
    d["unroll"] = gpu::copy_stream_unroll();
    return d;
  });
  // Tile plan of the production streaming kernel for n16 bulk elements
  // under a grid cap (0 = the process default). With `block`, also that
  // workgroup's tiles: first_tile, first_tile + grid, ..., last_tile
  // (n_tiles of them). Host-only.
  m.def("_copy_stream_plan",
        [](uint64_t n16, uint64_t stream_blocks, py::object block) {
          if (stream_blocks == 0)
            stream_blocks = gpu::copy_tuning().stream_blocks;
          if (stream_blocks == 0)
            throw py::value_error("copy_stream_plan: stream_blocks is 0");
          const StreamPlan p = stream_plan(
              n16, (uint32_t)gpu::copy_stream_unroll(), stream_blocks);
          py::dict d;
          d["tile"] = p.tile;
          d["full_tiles"] = p.full_tiles;
          d["ragged"] = p.ragged;
          d["tiles"] = p.tiles;
          d["grid"] = p.grid;
          if (!block.is_none()) {
            const StreamBlockTiles b =
                stream_block_tiles(p, block.cast<uint64_t>());
            d["first_tile"] = b.first;
            d["last_tile"] = b.last;
            d["n_tiles"] = b.count;
          }
          return d;
        },
        py::arg("n16"), py::arg("stream_blocks") = 0,
        py::arg("block") = py::none());
  // Test hooks for the small-message kernels (smallmsg.hip). They go
  // through the host functions the engine uses (inbox_create, same-process
  // inbox_push, inbox_unpack, arm_recv's two halves, arm_poll / arm_cancel
  // / arm_free / arm_leak); every wait has a ~2 s host deadline.
  py::class_<PyInboxRing>(m, "_InboxRing")
      .def(py::init([](uint32_t slots, uint32_t slot_bytes) {
             if (slots == 0 || slot_bytes < gpu::kInboxHdrBytes)
               throw py::value_error("_InboxRing: bad geometry");
             PyInboxRing r;
             r.info.slots = slots;
             r.info.slot_bytes = slot_bytes;
             return r;
           }),
           py::arg("slots"), py::arg("slot_bytes"))
      .def_property_readonly("slots",
                             [](const PyInboxRing& r) { return r.info.slots; })
      .def_property_readonly(
          "slot_bytes", [](const PyInboxRing& r) { return r.info.slot_bytes; })
      .def_property_readonly(
          "hdr_bytes", [](const PyInboxRing&) { return gpu::kInboxHdrBytes; })
      .def_property_readonly(
          "payload_max", [](const PyInboxRing& r) { return r.payload_max(); })
      .def_property_readonly("device",
                             [](const PyInboxRing& r) { return r.info.device; })
      .def_property_readonly("live",
                             [](const PyInboxRing& r) { return r.live; });
  py::class_<PyArmTicket>(m, "_InboxArmTicket");
  m.def("_inbox_ring_create",
        [](int device) {
          PyInboxRing r;
          released("inbox_ring_create", gpu::inbox_create, &r.info, device);
          r.live = true;
          return r;
        },
        py::arg("device"));
  m.def("_inbox_ring_destroy", [](PyInboxRing& r) {
    need_live(r, "inbox_ring_destroy");
    r.live = false;
    py::gil_scoped_release rel;
    gpu::inbox_destroy(r.info);
  });
  m.def("_inbox_ring_read", [](const PyInboxRing& r) {
    need_live(r, "inbox_ring_read");
    std::string out((size_t)r.info.slots * r.info.slot_bytes, '\0');
    released("inbox_ring_read", gpu::inbox_ring_read, r.info,
             (uint8_t*)out.data());
    return py::bytes(out);
  });
  m.def("_inbox_ring_write",
        [](const PyInboxRing& r, uint64_t offset, py::buffer data) {
          py::buffer_info bi = data.request();
          if (!PyBuffer_IsContiguous(bi.view(), 'C'))
            throw py::value_error("inbox_ring_write: data not contiguous");
          uint64_t n = (uint64_t)bi.size * (uint64_t)bi.itemsize;
          uint64_t total = (uint64_t)r.info.slots * r.info.slot_bytes;
          if (offset > total || n > total - offset)
            throw py::value_error("inbox_ring_write: out of range");
          need_live(r, "inbox_ring_write");
          released("inbox_ring_write", gpu::inbox_ring_write, r.info, offset,
                   (const uint8_t*)bi.ptr, n);
        },
        py::arg("ring"), py::arg("offset"), py::arg("data"));
  // msgs: list of (src_ptr, size, seq, tag); one k_inbox_push launch.
  m.def("_inbox_push_sync",
        [](const PyInboxRing& r,
           const std::vector<std::tuple<uintptr_t, uint64_t, uint64_t,
                                        uint64_t>>& msgs,
           int run_device) {
          check_inbox_batch("inbox_push_sync", msgs.size());
          gpu::PushMsg pm[32];
          for (size_t i = 0; i < msgs.size(); i++) {
            auto [src, size, seq, tag] = msgs[i];
            check_inbox_msg("inbox_push_sync", r, seq, size);
            pm[i] = gpu::PushMsg{(const uint8_t*)src, (uint32_t)size, seq, tag};
          }
          need_live(r, "inbox_push_sync");
          released("inbox_push_sync", gpu::inbox_push_sync, r.info, pm,
                   (int)msgs.size(), run_device);
        },
        py::arg("ring"), py::arg("msgs"), py::arg("run_device"));
  // msgs: list of (seq, size, dst_ptr or 0); one k_inbox_unpack launch.
  // Returns [(status, bounce bytes or None)]: status 1 delivered, 2 the
  // payload never arrived within the kernel's spin bound.
  m.def("_inbox_unpack_sync",
        [](const PyInboxRing& r,
           const std::vector<std::tuple<uint64_t, uint64_t, uintptr_t>>&
               msgs) {
          check_inbox_batch("inbox_unpack_sync", msgs.size());
          gpu::UnpackMsg um[32];
          for (size_t i = 0; i < msgs.size(); i++) {
            auto [seq, size, dst] = msgs[i];
            check_inbox_msg("inbox_unpack_sync", r, seq, size);
            um[i] = gpu::UnpackMsg{seq, (uint32_t)size, (uint8_t*)dst};
          }
          need_live(r, "inbox_unpack_sync");
          int status[32];
          std::vector<uint8_t> bounce[32];
          released("inbox_unpack_sync", gpu::inbox_unpack_sync, r.info, um,
                   (int)msgs.size(), status, bounce);
          py::list out;
          for (size_t i = 0; i < msgs.size(); i++) {
            py::object b = py::none();
            if (!um[i].dst)
              b = py::bytes((const char*)bounce[i].data(), bounce[i].size());
            out.append(py::make_tuple(status[i], b));
          }
          return out;
        },
        py::arg("ring"), py::arg("msgs"));
  m.def("_inbox_arm_begin",
        [](const PyInboxRing& r, uint64_t expect_seq, uint64_t tag,
           uint64_t mask, uintptr_t dst, uint64_t max_size,
           unsigned spin_iters, bool precancel) {
          // max_size is the buffer's capacity, not a message size: only
          // what is pushed is bounded by the slot.
          check_inbox_msg("inbox_arm_begin", r, expect_seq, 0);
          need_live(r, "inbox_arm_begin");
          PyArmTicket t;
          t.ticket = released("inbox_arm_begin", gpu::arm_begin, r.info,
                              expect_seq, tag, mask, (uint8_t*)dst, max_size,
                              spin_iters, precancel);
          return t;
        },
        py::arg("ring"), py::arg("expect_seq"), py::arg("tag"),
        py::arg("mask"), py::arg("dst"), py::arg("max_size"),
        py::arg("spin_iters") = 0, py::arg("precancel") = false);
  // (status, size): 0 running / 1 copied / 2 nomatch / 3 canceled /
  // 4 expired; size is the message's, non-zero with status 1 only.
  m.def("_inbox_arm_poll", [](const PyArmTicket& t) {
    need_ticket(t, "inbox_arm_poll");
    uint64_t size = 0;
    int st = gpu::arm_poll(t.ticket, &size);
    return py::make_tuple(st, size);
  });
  m.def("_inbox_arm_cancel", [](const PyArmTicket& t) {
    need_ticket(t, "inbox_arm_cancel");
    gpu::arm_cancel(t.ticket);
  });
  // Waits for a verdict, frees the ticket, returns (status, size).
  m.def("_inbox_arm_end", [](PyArmTicket& t) {
    need_ticket(t, "inbox_arm_end");
    void* ticket = t.ticket;
    t.ticket = nullptr;  // freed or leaked below, never reusable
    int st = 0;
    uint64_t size = 0;
    released("inbox_arm_end", gpu::arm_end, ticket, &st, &size);
    return py::make_tuple(st, size);
  });
}

}  // namespace sw
