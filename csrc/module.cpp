// starway_amd._core — Python bindings.
//
// Class/method surface mirrors the reference's nanobind module signature for
// signature (reference src/starway/_bindings.pyi is the contract), with one
// extension: buffers may be host arrays (buffer protocol) OR device tensors
// (__cuda_array_interface__, e.g. torch HIP tensors) — the reference was
// CPU-only (nb::device::cpu, main.hpp:155) and left GPU "planned".
#include "core.hpp"
#include "copy_stream.hpp"

#include <algorithm>

#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

namespace sw {

namespace gpu {
int device_of(const void* ptr);  // gpu_ptr.cpp helper
}

// Parse a message buffer into (ptr, nbytes, device). Host path uses the
// buffer protocol (zero-copy, C-contiguous); device path uses
// __cuda_array_interface__ (torch ROCm tensors export it).
static BufferRef parse_buffer(py::handle obj, bool writable) {
  BufferRef ref;
  if (py::hasattr(obj, "__cuda_array_interface__")) {
    py::dict cai = obj.attr("__cuda_array_interface__").cast<py::dict>();
    py::tuple data = cai["data"].cast<py::tuple>();
    uintptr_t ptr = data[0].cast<uintptr_t>();
    bool readonly = data[1].cast<bool>();
    if (writable && readonly)
      throw std::invalid_argument("recv buffer is read-only");
    py::tuple shape = cai["shape"].cast<py::tuple>();
    std::string typestr = cai["typestr"].cast<std::string>();
    size_t itemsize = std::stoul(typestr.substr(2));
    size_t n = 1;
    for (auto d : shape) n *= d.cast<size_t>();
    uint64_t rows = 0, row_bytes = 0, row_stride = 0;
    Layout nd{};
    if (cai.contains("strides") && !cai["strides"].is_none()) {
      py::tuple strides = cai["strides"].cast<py::tuple>();
      for (auto st : strides)
        if (st.cast<int64_t>() < 0)
          throw std::invalid_argument(
              "N-D layout limit: negative strides are not supported");
      size_t expect = itemsize;
      bool contiguous = true;
      for (ssize_t i = (ssize_t)shape.size() - 1; i >= 0; --i) {
        if (strides[i].cast<size_t>() != expect) contiguous = false;
        expect *= shape[i].cast<size_t>();
      }
      if (!contiguous) {
        // 2D row-strided layout is supported natively (pack/unpack in the
        // pull kernel): last dim dense, leading dim strided.
        if (shape.size() == 2 && strides[1].cast<size_t>() == itemsize &&
            strides[0].cast<uint64_t>() >=
                shape[1].cast<uint64_t>() * itemsize) {
          rows = shape[0].cast<uint64_t>();
          row_bytes = shape[1].cast<uint64_t>() * itemsize;
          row_stride = strides[0].cast<uint64_t>();
        } else if (n > 0) {
          // Any other view: normalise it. What comes out as contiguous or
          // as rows over a dense run keeps the fields (and kernels) above;
          // the rest travels as an N-D layout.
          std::vector<uint64_t> sh;
          std::vector<int64_t> st;
          for (size_t i = 0; i < shape.size(); i++) {
            sh.push_back(shape[i].cast<uint64_t>());
            st.push_back(strides[i].cast<int64_t>());
          }
          Layout l = normalize(sh.data(), st.data(), sh.size(), itemsize);
          if (l.ndim == 1 && l.stride[0] >= (int64_t)l.unit) {
            rows = l.shape[0];
            row_bytes = l.unit;
            row_stride = (uint64_t)l.stride[0];
          } else if (l.ndim > 0) {
            if (writable) check_no_overlap(l);
            nd = l;
          }
        }
      }
    }
    ref.ptr = (uint8_t*)ptr;
    ref.size = n * itemsize;
    if (nd.ndim > 0) {
      ref.nd = nd;
    } else if (rows > 1) {
      ref.rows = rows;
      ref.row_bytes = row_bytes;
      ref.stride = row_stride;
    }
    ref.device = gpu::device_of((const void*)ptr);
    if (ref.device < 0)
      throw std::invalid_argument(
          "buffer exports __cuda_array_interface__ but is not resident on a "
          "visible HIP device");
    return ref;
  }
  Py_buffer view;
  int flags = PyBUF_C_CONTIGUOUS | (writable ? PyBUF_WRITABLE : PyBUF_SIMPLE);
  if (PyObject_GetBuffer(obj.ptr(), &view, flags) != 0)
    throw py::error_already_set();
  ref.ptr = (uint8_t*)view.buf;
  ref.size = (size_t)view.len;
  ref.device = -1;
  PyBuffer_Release(&view);  // the keepalive object pins the memory
  return ref;
}

static ElemType parse_elem_type(const std::string& dtype) {
  if (dtype == "float32") return ElemType::F32;
  if (dtype == "float16") return ElemType::F16;
  if (dtype == "bfloat16") return ElemType::BF16;
  if (dtype == "int32") return ElemType::I32;
  return ElemType::None;
}

// recv(reduce=..., dtype=...). The op is checked before the buffer is
// looked at; everything else against the parsed buffer. Every refusal is a
// ValueError naming the limit.
static void check_reduce_op(const std::string& reduce) {
  if (!reduce.empty() && reduce != "sum")
    throw py::value_error("reduce limit: unknown op '" + reduce +
                          "' (supported: 'sum')");
}

static void apply_reduce(BufferRef& ref, const std::string& reduce,
                         const std::string& dtype) {
  if (reduce.empty()) return;
  if (ref.device < 0)
    throw py::value_error(
        "reduce limit: host buffers are not supported (device tensors only)");
  const ElemType et = parse_elem_type(dtype);
  if (et == ElemType::None)
    throw py::value_error("reduce limit: unsupported dtype '" + dtype +
                          "' (supported: float32, float16, bfloat16, int32)");
  if (!ref.dense())
    throw py::value_error(
        "reduce limit: the destination must be contiguous (strided and N-D "
        "views are not supported)");
  if ((uintptr_t)ref.ptr % elem_size(et))
    throw py::value_error("reduce limit: the destination must be aligned to "
                          "its item size (" +
                          std::to_string(elem_size(et)) + " B)");
  ref.reduce = ReduceOp::Sum;
  ref.elem = et;
}

// index= of send/recv: a host-side list of slice numbers along the
// buffer's first dimension (index.hpp). Every refusal is a ValueError whose
// text starts with "index limit:".
static py::value_error index_limit(const std::string& what) {
  return py::value_error("index limit: " + what);
}

// Validate and copy an index argument: a sequence of Python ints, a 1-D
// numpy integer array or a 1-D CPU torch integer tensor.
static std::shared_ptr<const IndexList> parse_index(py::object index,
                                                    uint64_t extent,
                                                    bool writable) {
  if (py::hasattr(index, "is_cuda")) {  // a torch tensor
    if (index.attr("is_cuda").cast<bool>())
      throw index_limit("the index must live on the host (reading a device "
                        "tensor would need a device synchronise)");
    index = index.attr("numpy")();
  } else if (py::hasattr(index, "__cuda_array_interface__")) {
    throw index_limit("the index must live on the host (reading a device "
                      "tensor would need a device synchronise)");
  }
  std::vector<int64_t> vals;
  if (py::isinstance<py::array>(index)) {
    py::array arr = py::reinterpret_borrow<py::array>(index);
    const char kind = arr.dtype().kind();
    if (kind != 'i' && kind != 'u')
      throw index_limit(std::string("the index must hold integers, not ") +
                        (kind == 'b' ? "bool" : kind == 'f' ? "float"
                                                            : "this dtype"));
    if (arr.ndim() != 1)
      throw index_limit("the index must be 1-D, not " +
                        std::to_string(arr.ndim()) + "-D");
    if (kind == 'u' && arr.itemsize() == 8) {
      // Above int64 is out of range for any buffer; keep it positive.
      auto u = py::array_t<uint64_t, py::array::c_style |
                                         py::array::forcecast>(arr);
      for (ssize_t i = 0; i < u.size(); i++)
        vals.push_back((int64_t)std::min<uint64_t>(u.data()[i], INT64_MAX));
    } else {
      auto a = py::array_t<int64_t, py::array::c_style |
                                        py::array::forcecast>(arr);
      vals.assign(a.data(), a.data() + a.size());
    }
  } else if (py::isinstance<py::sequence>(index) &&
             !py::isinstance<py::str>(index) &&
             !py::isinstance<py::bytes>(index)) {
    py::sequence seq = py::reinterpret_borrow<py::sequence>(index);
    for (py::handle h : seq) {
      if (py::isinstance<py::bool_>(h))
        throw index_limit("the index must hold integers, not bool");
      if (py::isinstance<py::float_>(h))
        throw index_limit("the index must hold integers, not float");
      if (!py::isinstance<py::int_>(h) && !py::hasattr(h, "__index__"))
        throw index_limit("the index must be 1-D and hold integers");
      int overflow = 0;
      py::object as_int = py::reinterpret_steal<py::object>(
          PyNumber_Index(h.ptr()));
      if (!as_int) throw py::error_already_set();
      long long v = PyLong_AsLongLongAndOverflow(as_int.ptr(), &overflow);
      if (overflow) v = overflow < 0 ? INT64_MIN : INT64_MAX;
      vals.push_back((int64_t)v);
    }
  } else {
    throw index_limit("the index must be a sequence of ints, a 1-D numpy "
                      "integer array or a 1-D CPU torch integer tensor");
  }
  return plan_index(vals.data(), vals.size(), extent, writable);
}

// A message buffer with index=: the device tensor's own geometry (shape and
// byte strides as they are, not merged), of which the first dimension is
// indexed and the rest must be dense, so each slice buf[i] is one run.
static BufferRef parse_indexed_buffer(py::handle obj, py::object index,
                                      bool writable) {
  if (!py::hasattr(obj, "__cuda_array_interface__")) {
    // A host buffer is refused whatever the index; a bad index is still
    // named first, so its message does not depend on where the buffer is.
    Py_buffer view;
    if (PyObject_GetBuffer(obj.ptr(), &view, PyBUF_STRIDES) == 0) {
      const bool has_dim = view.ndim >= 1;
      const uint64_t extent = has_dim ? (uint64_t)view.shape[0] : 0;
      PyBuffer_Release(&view);
      if (has_dim) parse_index(index, extent, writable);
    } else {
      PyErr_Clear();
    }
    throw index_limit("host buffers are not supported (device tensors only)");
  }
  py::dict cai = obj.attr("__cuda_array_interface__").cast<py::dict>();
  py::tuple data = cai["data"].cast<py::tuple>();
  const uintptr_t ptr = data[0].cast<uintptr_t>();
  if (writable && data[1].cast<bool>())
    throw std::invalid_argument("recv buffer is read-only");
  py::tuple shape = cai["shape"].cast<py::tuple>();
  const std::string typestr = cai["typestr"].cast<std::string>();
  const uint64_t itemsize = std::stoul(typestr.substr(2));
  if (shape.size() < 1)
    throw index_limit("the buffer needs at least one dimension");
  const uint64_t extent = shape[0].cast<uint64_t>();
  uint64_t slice_bytes = itemsize;
  for (size_t i = 1; i < shape.size(); i++)
    slice_bytes *= shape[i].cast<uint64_t>();
  uint64_t stride = slice_bytes;
  if (cai.contains("strides") && !cai["strides"].is_none()) {
    py::tuple strides = cai["strides"].cast<py::tuple>();
    uint64_t expect = itemsize;
    for (ssize_t i = (ssize_t)shape.size() - 1; i >= 1; --i) {
      const uint64_t extent_i = shape[i].cast<uint64_t>();
      if (extent_i != 1 && strides[i].cast<int64_t>() != (int64_t)expect)
        throw index_limit("the buffer's slices must be dense (dimensions "
                          "after the first contiguous among themselves)");
      expect *= extent_i;
    }
    const int64_t s0 = strides[0].cast<int64_t>();
    if (s0 < 0)
      throw index_limit("negative strides are not supported");
    stride = (uint64_t)s0;
  }
  if (writable && extent > 1 && stride < slice_bytes)
    throw index_limit("a destination's slices must not overlap (stride " +
                      std::to_string(stride) + " B under a slice of " +
                      std::to_string(slice_bytes) + " B)");
  BufferRef ref;
  ref.index.list = parse_index(std::move(index), extent, writable);
  // The peer's decoder refuses a list of empty slices as malformed; refuse
  // it here, where the caller sees why.
  if (slice_bytes == 0 && ref.index.count() > 0)
    throw index_limit("the buffer's slices are empty (a dimension after "
                      "the first has extent 0)");
  ref.index.slice_bytes = slice_bytes;
  ref.index.stride = stride;
  ref.ptr = (uint8_t*)ptr;
  ref.size = (size_t)(ref.index.count() * slice_bytes);
  ref.device = gpu::device_of((const void*)ptr);
  if (ref.device < 0)
    throw std::invalid_argument(
        "buffer exports __cuda_array_interface__ but is not resident on a "
        "visible HIP device");
  return ref;
}

// The buffer of a send (reduce empty) or recv, with or without index=.
static BufferRef parse_message_buffer(py::handle buffer, py::object index,
                                      bool writable,
                                      const std::string& reduce = "",
                                      const std::string& dtype = "") {
  check_reduce_op(reduce);
  if (index.is_none()) {
    BufferRef ref = parse_buffer(buffer, writable);
    apply_reduce(ref, reduce, dtype);
    return ref;
  }
  if (!reduce.empty())
    throw index_limit("index= cannot be combined with reduce= (a reducing "
                      "destination stays contiguous)");
  return parse_indexed_buffer(buffer, std::move(index), writable);
}

// One side of _copy_index_sync: None for a dense side.
static IndexRef hook_index_side(py::object index, uint64_t slice_bytes,
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

static Plan plan_of(const Layout& l) {
  Plan p;
  p.first = l.unit;
  for (uint32_t d = 0; d < l.ndim; d++)
    p.second.emplace_back(l.shape[d], l.stride[d]);
  return p;
}

static Layout layout_of(const Plan& p) {
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

static Layout layout_from(const std::vector<uint64_t>& shape,
                          const std::vector<int64_t>& strides,
                          uint64_t itemsize, bool writable) {
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

static void need_live(const PyInboxRing& r, const char* what) {
  if (!r.live)
    throw std::runtime_error(std::string(what) +
                             ": ring has no device memory (detached or "
                             "destroyed)");
}

static void check_inbox_batch(const char* what, size_t n) {
  if (n < 1 || n > 32)
    throw py::value_error(std::string(what) + ": need 1..32 descriptors");
}

static void check_inbox_msg(const char* what, const PyInboxRing& r,
                            uint64_t seq, uint64_t size) {
  if (seq == 0)
    throw py::value_error(std::string(what) +
                          ": seq 0 is the empty-slot sentinel");
  if (size > r.payload_max())
    throw py::value_error(std::string(what) + ": size " +
                          std::to_string(size) + " exceeds payload_max " +
                          std::to_string(r.payload_max()));
}

struct PyServer {
  Engine engine{Engine::ServerMode};
  explicit PyServer(Context&) {
    engine.preferred_device_ = gpu::current_device();
  }
};

struct PyClient {
  Engine engine{Engine::ClientMode};
  explicit PyClient(Context&) {
    engine.preferred_device_ = gpu::current_device();
  }
};

}  // namespace sw

using namespace sw;

PYBIND11_MODULE(_core, m) {
  m.doc() =
      "starway_amd native core: MI355X-native tagged async zero-copy "
      "messaging (TCP control plane + hipIpc/xGMI data plane with gfx950 "
      "copy kernels)";

  py::class_<Context>(m, "Context").def(py::init<>());

  py::class_<EndpointInfo, std::shared_ptr<EndpointInfo>>(m, "ServerEndpoint")
      .def_property_readonly("name",
                             [](const EndpointInfo& e) { return e.name; })
      .def_property_readonly(
          "local_addr", [](const EndpointInfo& e) { return e.local_addr; })
      .def_property_readonly(
          "local_port", [](const EndpointInfo& e) { return e.local_port; })
      .def_property_readonly(
          "remote_addr", [](const EndpointInfo& e) { return e.remote_addr; })
      .def_property_readonly(
          "remote_port", [](const EndpointInfo& e) { return e.remote_port; })
      .def("view_transports",
           [](const EndpointInfo& e) { return e.transports; })
      .def("__eq__",
           [](const EndpointInfo& a, py::object other) {
             if (!py::isinstance<EndpointInfo>(other)) return false;
             return &a == other.cast<EndpointInfo*>();
           })
      .def("__hash__",
           [](const EndpointInfo& e) { return (size_t)(uintptr_t)&e; })
      .def("__repr__", [](const EndpointInfo& e) {
        return "<ServerEndpoint " + e.name + ">";
      });

  py::class_<PyServer>(m, "Server")
      .def(py::init<Context&>(), py::arg("ctx"), py::keep_alive<1, 2>())
      .def("set_accept_callback",
           [](PyServer& s, py::object cb) {
             s.engine.set_accept_callback(std::move(cb));
           },
           py::arg("callback"))
      .def("listen",
           [](PyServer& s, const std::string& addr, int port) {
             s.engine.listen(addr, port);
           },
           py::arg("addr"), py::arg("port"))
      .def("listen_address", [](PyServer& s) { s.engine.listen_address(); })
      .def("get_worker_address",
           [](PyServer& s) {
             auto v = s.engine.get_worker_address();
             return py::bytes((const char*)v.data(), v.size());
           })
      .def("close",
           [](PyServer& s, py::object cb) { s.engine.close(std::move(cb)); },
           py::arg("callback"))
      .def("send",
           [](PyServer& s, std::shared_ptr<EndpointInfo> ep, py::object buffer,
              uint64_t tag, py::object done, py::object fail,
              py::object index) {
             BufferRef ref = parse_message_buffer(buffer, std::move(index),
                                                  /*writable=*/false);
             s.engine.send(std::move(ep), ref, tag, std::move(done),
                           std::move(fail), std::move(buffer));
           },
           py::arg("client_ep"), py::arg("buffer"), py::arg("tag"),
           py::arg("done_callback"), py::arg("fail_callback"),
           py::arg("index") = py::none())
      .def("recv",
           [](PyServer& s, py::object buffer, uint64_t tag, uint64_t tag_mask,
              py::object done, py::object fail, const std::string& reduce,
              const std::string& dtype, py::object index) {
             BufferRef ref = parse_message_buffer(
                 buffer, std::move(index), /*writable=*/true, reduce, dtype);
             s.engine.recv(ref, tag, tag_mask, std::move(done),
                           std::move(fail), std::move(buffer));
           },
           py::arg("buffer"), py::arg("tag"), py::arg("tag_mask"),
           py::arg("done_callback"), py::arg("fail_callback"),
           py::arg("reduce") = "", py::arg("dtype") = "",
           py::arg("index") = py::none())
      .def("flush",
           [](PyServer& s, py::object done, py::object fail) {
             s.engine.flush(std::move(done), std::move(fail));
           },
           py::arg("done_callback"), py::arg("fail_callback"))
      .def("flush_ep",
           [](PyServer& s, std::shared_ptr<EndpointInfo> ep, py::object done,
              py::object fail) {
             s.engine.flush_ep(std::move(ep), std::move(done),
                               std::move(fail));
           },
           py::arg("client_ep"), py::arg("done_callback"),
           py::arg("fail_callback"))
      .def("get_stats",
           [](PyServer& s) {
             py::dict d;
             auto& st = s.engine.stats_;
             d["msgs_sent"] = st.msgs_sent.load();
             d["msgs_received"] = st.msgs_received.load();
             d["bytes_sent"] = st.bytes_sent.load();
             d["bytes_received"] = st.bytes_received.load();
             d["eager_rx"] = st.eager_rx.load();
             d["gpu_rx"] = st.gpu_rx.load();
             d["cma_rx"] = st.cma_rx.load();
             d["unexpected_rx"] = st.unexpected_rx.load();
             d["unexp_staged_bytes"] = st.unexp_staged_bytes.load();
             d["deferred_sends"] = st.deferred_sends.load();
             d["inbox_rx"] = st.inbox_rx.load();
             d["inbox_tx"] = st.inbox_tx.load();
             d["doorbell_rx"] = st.doorbell_rx.load();
             d["reduce_rx"] = st.reduce_rx.load();
             d["index_tx"] = st.index_tx.load();
             d["index_rx"] = st.index_rx.load();
             return d;
           })
      .def("list_clients",
           [](PyServer& s) {
             py::set out;
             for (auto& ep : s.engine.list_clients()) out.add(py::cast(ep));
             return out;
           })
      .def("evaluate_perf",
           [](PyServer& s, std::shared_ptr<EndpointInfo> ep,
              uint64_t msg_size) {
             return s.engine.evaluate_perf(std::move(ep), msg_size);
           },
           py::arg("client_ep"), py::arg("msg_size"));

  py::class_<PyClient>(m, "Client")
      .def(py::init<Context&>(), py::arg("ctx"), py::keep_alive<1, 2>())
      .def("connect",
           [](PyClient& c, const std::string& addr, int port, py::object cb) {
             c.engine.connect(addr, port, std::move(cb));
           },
           py::arg("addr"), py::arg("port"), py::arg("callback"))
      .def("connect_address",
           [](PyClient& c, py::bytes blob, py::object cb) {
             std::string s = blob;
             std::vector<uint8_t> v(s.begin(), s.end());
             c.engine.connect_address(v, std::move(cb));
           },
           py::arg("remote_address"), py::arg("callback"))
      .def("get_worker_address",
           [](PyClient& c) {
             auto v = c.engine.get_worker_address();
             return py::bytes((const char*)v.data(), v.size());
           })
      .def("close",
           [](PyClient& c, py::object cb) { c.engine.close(std::move(cb)); },
           py::arg("callback"))
      .def("send",
           [](PyClient& c, py::object buffer, uint64_t tag, py::object done,
              py::object fail, py::object index) {
             BufferRef ref = parse_message_buffer(buffer, std::move(index),
                                                  /*writable=*/false);
             c.engine.send(nullptr, ref, tag, std::move(done),
                           std::move(fail), std::move(buffer));
           },
           py::arg("buffer"), py::arg("tag"), py::arg("done_callback"),
           py::arg("fail_callback"), py::arg("index") = py::none())
      .def("recv",
           [](PyClient& c, py::object buffer, uint64_t tag, uint64_t tag_mask,
              py::object done, py::object fail, const std::string& reduce,
              const std::string& dtype, py::object index) {
             BufferRef ref = parse_message_buffer(
                 buffer, std::move(index), /*writable=*/true, reduce, dtype);
             c.engine.recv(ref, tag, tag_mask, std::move(done),
                           std::move(fail), std::move(buffer));
           },
           py::arg("buffer"), py::arg("tag"), py::arg("tag_mask"),
           py::arg("done_callback"), py::arg("fail_callback"),
           py::arg("reduce") = "", py::arg("dtype") = "",
           py::arg("index") = py::none())
      .def("flush",
           [](PyClient& c, py::object done, py::object fail) {
             c.engine.flush(std::move(done), std::move(fail));
           },
           py::arg("done_callback"), py::arg("fail_callback"))
      .def("get_stats",
           [](PyClient& c) {
             py::dict d;
             auto& st = c.engine.stats_;
             d["msgs_sent"] = st.msgs_sent.load();
             d["msgs_received"] = st.msgs_received.load();
             d["bytes_sent"] = st.bytes_sent.load();
             d["bytes_received"] = st.bytes_received.load();
             d["eager_rx"] = st.eager_rx.load();
             d["gpu_rx"] = st.gpu_rx.load();
             d["cma_rx"] = st.cma_rx.load();
             d["unexpected_rx"] = st.unexpected_rx.load();
             d["unexp_staged_bytes"] = st.unexp_staged_bytes.load();
             d["deferred_sends"] = st.deferred_sends.load();
             d["inbox_rx"] = st.inbox_rx.load();
             d["inbox_tx"] = st.inbox_tx.load();
             d["doorbell_rx"] = st.doorbell_rx.load();
             d["reduce_rx"] = st.reduce_rx.load();
             d["index_tx"] = st.index_tx.load();
             d["index_rx"] = st.index_rx.load();
             return d;
           })
      .def("evaluate_perf", [](PyClient& c, uint64_t msg_size) {
        return c.engine.evaluate_perf(nullptr, msg_size);
      },
           py::arg("msg_size"));

  m.def("gpu_available", [] { return gpu::available(); });
  // Run (or re-run) the on-box copy microbenchmark backing evaluate_perf
  // and persist it to ~/.cache/starway/perf.cal (STARWAY_CALIB_FILE to
  // override). Returns {same_gpu_gbps, xgmi_gbps} in effect.
  m.def("calibrate",
        [](bool force) {
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::calibrate(force, &err);
          }
          if (!ok) throw std::runtime_error("calibrate: " + err);
          py::dict d;
          d["same_gpu_gbps"] = gpu::same_gpu_copy_gbps();
          d["xgmi_gbps"] = gpu::xgmi_link_gbps();
          return d;
        },
        py::arg("force") = false);
  m.def("gpu_device_count", [] { return gpu::device_count(); });
  // IPC hygiene: close every imported hipIpc mapping and drop the handle
  // caches. Call after returning GPU memory to the driver (e.g.
  // torch.cuda.empty_cache()) so a reused base address can never serve a
  // stale handle. Also registered as an atexit hook by the Python facade.
  m.def("ipc_invalidate", [] {
    py::gil_scoped_release rel;
    gpu::ipc_close_all();
  });
  // Test/bench hooks: run the gfx950 copy kernels synchronously on raw
  // device pointers. Tuning arguments of 0 mean the process default
  // (_copy_tuning()); explicit values let one process reach every kernel
  // variant and a capped (multi-iteration) grid at small sizes.
  m.def("_copy_device_sync",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, int device,
           size_t block_cap, size_t nt_threshold, int nt_unroll,
           size_t stream_threshold, size_t stream_blocks) {
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::copy_device_sync(
                (void*)dst, (const void*)src, nbytes, device,
                CopyTuning{block_cap, nt_threshold, nt_unroll,
                           stream_threshold, stream_blocks},
                &err);
          }
          if (!ok) throw std::runtime_error("copy_device_sync: " + err);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("device"),
        py::arg("block_cap") = 0, py::arg("nt_threshold") = 0,
        py::arg("nt_unroll") = 0, py::arg("stream_threshold") = 0,
        py::arg("stream_blocks") = 0);
  m.def("_copy_strided_sync",
        [](uintptr_t dst, uint64_t dst_stride, uintptr_t src,
           uint64_t src_stride, uint64_t rows, uint64_t row_bytes, int device,
           size_t block_cap) {
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::copy_strided_sync((void*)dst, dst_stride,
                                        (const void*)src, src_stride, rows,
                                        row_bytes, device, block_cap, &err);
          }
          if (!ok) throw std::runtime_error("copy_strided_sync: " + err);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::accum_sync((void*)dst, (const void*)src, nbytes, et,
                                 device,
                                 CopyTuning{block_cap, 0, 0, 0, 0, nt_threshold},
                                 &err);
          }
          if (!ok) throw std::runtime_error("accum_sync: " + err);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("dtype"),
        py::arg("device"), py::arg("block_cap") = 0,
        py::arg("nt_threshold") = 0);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::copy_multi_sync(d, (int)descs.size(), device, &err);
          }
          if (!ok) throw std::runtime_error("copy_multi_sync: " + err);
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
           int device, size_t block_cap, const std::string& path) {
          CopyNdPath p;
          if (path == "auto") p = CopyNdPath::Auto;
          else if (path == "generic") p = CopyNdPath::Generic;
          else if (path == "tiled") p = CopyNdPath::Tiled;
          else throw py::value_error("copy_nd_sync: path must be auto, "
                                     "generic or tiled");
          uint64_t dbytes = itemsize, sbytes = itemsize;
          for (uint64_t e : dst_shape) dbytes *= e;
          for (uint64_t e : src_shape) sbytes *= e;
          if (dbytes != sbytes)
            throw py::value_error("copy_nd_sync: source holds " +
                                  std::to_string(sbytes) +
                                  " B, destination " + std::to_string(dbytes));
          Layout dl = layout_from(dst_shape, dst_strides, itemsize, true);
          Layout sl = layout_from(src_shape, src_strides, itemsize, false);
          std::string err;
          bool ok, ineligible = false;
          {
            py::gil_scoped_release rel;
            ok = gpu::copy_nd_sync((void*)dst, dl, (const void*)src, sl,
                                   sbytes, device, block_cap, p, &ineligible,
                                   &err);
          }
          if (ineligible) throw py::value_error("copy_nd_sync: " + err);
          if (!ok) throw std::runtime_error("copy_nd_sync: " + err);
        },
        py::arg("dst"), py::arg("dst_shape"), py::arg("dst_strides"),
        py::arg("src"), py::arg("src_shape"), py::arg("src_strides"),
        py::arg("itemsize"), py::arg("device"), py::arg("block_cap") = 0,
        py::arg("path") = "auto");
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
  m.def("_copy_index_sync",
        [](uintptr_t dst, py::object dst_index, uint64_t dst_slice,
           uint64_t dst_stride, uintptr_t src, py::object src_index,
           uint64_t src_slice, uint64_t src_stride, uint64_t bytes, int device,
           size_t block_cap) {
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::copy_index_sync((void*)dst, di, (const void*)src, si,
                                      bytes, device, block_cap, &err);
          }
          if (!ok) throw std::runtime_error("copy_index_sync: " + err);
        },
        py::arg("dst"), py::arg("dst_index"), py::arg("dst_slice"),
        py::arg("dst_stride"), py::arg("src"), py::arg("src_index"),
        py::arg("src_slice"), py::arg("src_stride"), py::arg("bytes"),
        py::arg("device"), py::arg("block_cap") = 0);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::inbox_create(&r.info, device, &err);
          }
          if (!ok) throw std::runtime_error("inbox_ring_create: " + err);
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
    std::string err;
    bool ok;
    {
      py::gil_scoped_release rel;
      ok = gpu::inbox_ring_read(r.info, (uint8_t*)out.data(), &err);
    }
    if (!ok) throw std::runtime_error("inbox_ring_read: " + err);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::inbox_ring_write(r.info, offset,
                                       (const uint8_t*)bi.ptr, n, &err);
          }
          if (!ok) throw std::runtime_error("inbox_ring_write: " + err);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::inbox_push_sync(r.info, pm, (int)msgs.size(),
                                      run_device, &err);
          }
          if (!ok) throw std::runtime_error("inbox_push_sync: " + err);
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
          std::string err;
          bool ok;
          {
            py::gil_scoped_release rel;
            ok = gpu::inbox_unpack_sync(r.info, um, (int)msgs.size(), status,
                                        bounce, &err);
          }
          if (!ok) throw std::runtime_error("inbox_unpack_sync: " + err);
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
          std::string err;
          PyArmTicket t;
          {
            py::gil_scoped_release rel;
            t.ticket = gpu::arm_begin(r.info, expect_seq, tag, mask,
                                      (uint8_t*)dst, max_size, spin_iters,
                                      precancel, &err);
          }
          if (!t.ticket) throw std::runtime_error("inbox_arm_begin: " + err);
          return t;
        },
        py::arg("ring"), py::arg("expect_seq"), py::arg("tag"),
        py::arg("mask"), py::arg("dst"), py::arg("max_size"),
        py::arg("spin_iters") = 0, py::arg("precancel") = false);
  auto need_ticket = [](const PyArmTicket& t, const char* what) {
    if (!t.ticket)
      throw std::runtime_error(std::string(what) + ": ticket already ended");
  };
  // (status, size): 0 running / 1 copied / 2 nomatch / 3 canceled /
  // 4 expired; size is the message's, non-zero with status 1 only.
  m.def("_inbox_arm_poll", [need_ticket](const PyArmTicket& t) {
    need_ticket(t, "inbox_arm_poll");
    uint64_t size = 0;
    int st = gpu::arm_poll(t.ticket, &size);
    return py::make_tuple(st, size);
  });
  m.def("_inbox_arm_cancel", [need_ticket](const PyArmTicket& t) {
    need_ticket(t, "inbox_arm_cancel");
    gpu::arm_cancel(t.ticket);
  });
  // Waits for a verdict, frees the ticket, returns (status, size).
  m.def("_inbox_arm_end", [need_ticket](PyArmTicket& t) {
    need_ticket(t, "inbox_arm_end");
    void* ticket = t.ticket;
    t.ticket = nullptr;  // freed or leaked below, never reusable
    int st = 0;
    uint64_t size = 0;
    std::string err;
    bool ok;
    {
      py::gil_scoped_release rel;
      ok = gpu::arm_end(ticket, &st, &size, &err);
    }
    if (!ok) throw std::runtime_error("inbox_arm_end: " + err);
    return py::make_tuple(st, size);
  });
  m.attr("__version__") = "0.1.0";
}
