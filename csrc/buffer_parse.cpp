// Python object -> BufferRef. Runs on every send and recv.
//
// Buffers may be host arrays (buffer protocol) OR device tensors
// (__cuda_array_interface__, e.g. torch HIP tensors).
#include "buffer_parse.hpp"

#include <algorithm>

#include <pybind11/numpy.h>

namespace sw {

namespace gpu {
int device_of(const void* ptr);  // gpu.cpp
}

namespace {

// What an object's __cuda_array_interface__ says, read once: shape and
// byte strides as they are, not merged. Up to kInline dimensions live in
// the value itself; only a wider view allocates.
struct CudaArray {
  static constexpr size_t kInline = 8;
  uintptr_t ptr = 0;
  bool readonly = false;
  bool has_strides = false;  // false: C-contiguous, strides() unset
  size_t ndim = 0;
  uint64_t itemsize = 0;
  const uint64_t* shape() const { return wide.empty() ? dims : wide.data(); }
  const int64_t* strides() const {
    return wide.empty() ? steps : (const int64_t*)wide.data() + ndim;
  }
  uint64_t dims[kInline] = {};
  int64_t steps[kInline] = {};
  std::vector<uint64_t> wide;  // shape, then strides, when ndim > kInline
};

// A read-only array is refused for a recv here, before its shape is looked
// at.
CudaArray read_cuda_array(py::handle obj, bool writable) {
  CudaArray a;
  py::dict cai = obj.attr("__cuda_array_interface__").cast<py::dict>();
  py::tuple data = cai["data"].cast<py::tuple>();
  a.ptr = data[0].cast<uintptr_t>();
  a.readonly = data[1].cast<bool>();
  if (writable && a.readonly)
    throw std::invalid_argument("recv buffer is read-only");
  py::tuple shape = cai["shape"].cast<py::tuple>();
  const std::string typestr = cai["typestr"].cast<std::string>();
  a.itemsize = std::stoul(typestr.substr(2));
  a.ndim = shape.size();
  if (a.ndim > CudaArray::kInline) a.wide.resize(2 * a.ndim);
  uint64_t* sh = a.wide.empty() ? a.dims : a.wide.data();
  for (size_t i = 0; i < a.ndim; i++) sh[i] = shape[i].cast<uint64_t>();
  if (cai.contains("strides")) {
    py::object given = cai["strides"];
    if (!given.is_none()) {
      py::tuple strides = given.cast<py::tuple>();
      int64_t* st = a.wide.empty() ? a.steps : (int64_t*)a.wide.data() + a.ndim;
      for (size_t i = 0; i < a.ndim; i++) st[i] = strides[i].cast<int64_t>();
      a.has_strides = true;
    }
  }
  return a;
}

// The device a __cuda_array_interface__ pointer lives on. Raised last, after
// every layout and index refusal: those do not need a device to be named.
int resident_device(uintptr_t ptr) {
  const int device = gpu::device_of((const void*)ptr);
  if (device < 0)
    throw std::invalid_argument(
        "buffer exports __cuda_array_interface__ but is not resident on a "
        "visible HIP device");
  return device;
}

// Parse a message buffer into (ptr, nbytes, device). Host path uses the
// buffer protocol (zero-copy, C-contiguous); device path uses
// __cuda_array_interface__ (torch ROCm tensors export it).
BufferRef parse_buffer(py::handle obj, bool writable) {
  BufferRef ref;
  if (py::hasattr(obj, "__cuda_array_interface__")) {
    const CudaArray a = read_cuda_array(obj, writable);
    const uint64_t* shape = a.shape();
    const uint64_t itemsize = a.itemsize;
    size_t n = 1;
    for (size_t i = 0; i < a.ndim; i++) n *= shape[i];
    uint64_t rows = 0, row_bytes = 0, row_stride = 0;
    Layout nd{};
    if (a.has_strides) {
      const int64_t* strides = a.strides();
      for (size_t i = 0; i < a.ndim; i++)
        if (strides[i] < 0)
          throw std::invalid_argument(
              "N-D layout limit: negative strides are not supported");
      uint64_t expect = itemsize;
      bool contiguous = true;
      for (size_t i = a.ndim; i-- > 0;) {
        if ((uint64_t)strides[i] != expect) contiguous = false;
        expect *= shape[i];
      }
      if (!contiguous) {
        // 2D row-strided layout is supported natively (pack/unpack in the
        // pull kernel): last dim dense, leading dim strided. Not left to
        // normalize(): it refuses a row of 4 GiB or more, this does not.
        if (a.ndim == 2 && (uint64_t)strides[1] == itemsize &&
            (uint64_t)strides[0] >= shape[1] * itemsize) {
          rows = shape[0];
          row_bytes = shape[1] * itemsize;
          row_stride = (uint64_t)strides[0];
        } else if (n > 0) {
          // Any other view: normalise it. What comes out as contiguous or
          // as rows over a dense run keeps the fields (and kernels) above;
          // the rest travels as an N-D layout.
          Layout l = normalize(shape, strides, a.ndim, itemsize);
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
    ref.ptr = (uint8_t*)a.ptr;
    ref.size = n * itemsize;
    if (nd.ndim > 0) {
      ref.nd = nd;
    } else if (rows > 1) {
      ref.rows = rows;
      ref.row_bytes = row_bytes;
      ref.stride = row_stride;
    }
    ref.device = resident_device(a.ptr);
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

// recv(reduce=..., dtype=...). The op is checked before the buffer is
// looked at; everything else against the parsed buffer. Every refusal is a
// ValueError naming the limit.
void check_reduce_op(const std::string& reduce) {
  if (!reduce.empty() && reduce != "sum")
    throw py::value_error("reduce limit: unknown op '" + reduce +
                          "' (supported: 'sum')");
}

void apply_reduce(BufferRef& ref, const std::string& reduce,
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

// recv(msg_dtype=...): the element type of the message, when it is not the
// buffer's own. Every refusal is a ValueError whose text starts with
// "msg_dtype limit:". The name is checked before the buffer is looked at;
// everything else against the parsed buffer, after apply_reduce.
py::value_error msg_dtype_limit(const std::string& what) {
  return py::value_error("msg_dtype limit: " + what);
}

bool float_elem(ElemType t) {
  return t == ElemType::F32 || t == ElemType::F16 || t == ElemType::BF16;
}

void check_msg_dtype(const std::string& msg_dtype) {
  if (!msg_dtype.empty() && !float_elem(parse_elem_type(msg_dtype)))
    throw msg_dtype_limit("unsupported message dtype '" + msg_dtype +
                          "' (supported: float32, float16, bfloat16)");
}

void apply_msg_dtype(BufferRef& ref, const std::string& msg_dtype,
                     const std::string& dtype) {
  if (msg_dtype.empty()) return;
  if (ref.device < 0)
    throw msg_dtype_limit(
        "host buffers are not supported (device tensors only)");
  const ElemType et = parse_elem_type(dtype);
  if (!float_elem(et))
    throw msg_dtype_limit("unsupported buffer dtype '" + dtype +
                          "' (supported: float32, float16, bfloat16)");
  const ElemType mt = parse_elem_type(msg_dtype);
  // The buffer's own type: today's receive, plain or reducing.
  if (mt == et) return;
  if (!ref.dense())
    throw msg_dtype_limit(
        "the destination must be contiguous (strided and N-D views are not "
        "supported)");
  if ((uintptr_t)ref.ptr % elem_size(et))
    throw msg_dtype_limit("the destination must be aligned to its item "
                          "size (" +
                          std::to_string(elem_size(et)) + " B)");
  ref.elem = et;
  ref.msg_elem = mt;
}

// index= of send/recv: a host-side list of slice numbers along the
// buffer's first dimension (index.hpp). Every refusal is a ValueError whose
// text starts with "index limit:".
py::value_error index_limit(const std::string& what) {
  return py::value_error("index limit: " + what);
}

// A message buffer with index=: the device tensor's own geometry, of which
// the first dimension is indexed and the rest must be dense, so each slice
// buf[i] is one run.
BufferRef parse_indexed_buffer(py::handle obj, py::object index,
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
  const CudaArray a = read_cuda_array(obj, writable);
  const uint64_t* shape = a.shape();
  if (a.ndim < 1)
    throw index_limit("the buffer needs at least one dimension");
  const uint64_t extent = shape[0];
  uint64_t slice_bytes = a.itemsize;
  for (size_t i = 1; i < a.ndim; i++) slice_bytes *= shape[i];
  uint64_t stride = slice_bytes;
  if (a.has_strides) {
    const int64_t* strides = a.strides();
    uint64_t expect = a.itemsize;
    for (size_t i = a.ndim - 1; i >= 1; --i) {
      if (shape[i] != 1 && strides[i] != (int64_t)expect)
        throw index_limit("the buffer's slices must be dense (dimensions "
                          "after the first contiguous among themselves)");
      expect *= shape[i];
    }
    if (strides[0] < 0)
      throw index_limit("negative strides are not supported");
    stride = (uint64_t)strides[0];
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
  ref.ptr = (uint8_t*)a.ptr;
  ref.size = (size_t)(ref.index.count() * slice_bytes);
  ref.device = resident_device(a.ptr);
  return ref;
}

}  // namespace

ElemType parse_elem_type(const std::string& dtype) {
  if (dtype == "float32") return ElemType::F32;
  if (dtype == "float16") return ElemType::F16;
  if (dtype == "bfloat16") return ElemType::BF16;
  if (dtype == "int32") return ElemType::I32;
  return ElemType::None;
}

std::shared_ptr<const IndexList> parse_index(py::object index, uint64_t extent,
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

BufferRef parse_message_buffer(py::handle buffer, py::object index,
                               bool writable, const std::string& reduce,
                               const std::string& dtype,
                               const std::string& msg_dtype) {
  check_reduce_op(reduce);
  check_msg_dtype(msg_dtype);
  if (index.is_none()) {
    BufferRef ref = parse_buffer(buffer, writable);
    apply_reduce(ref, reduce, dtype);
    apply_msg_dtype(ref, msg_dtype, dtype);
    return ref;
  }
  if (!msg_dtype.empty())
    throw msg_dtype_limit("index= cannot be combined with msg_dtype= (a "
                          "converting destination stays contiguous)");
  if (!reduce.empty())
    throw index_limit("index= cannot be combined with reduce= (a reducing "
                      "destination stays contiguous)");
  return parse_indexed_buffer(buffer, std::move(index), writable);
}

}  // namespace sw
