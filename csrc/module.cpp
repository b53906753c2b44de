// starway_amd._core — Python bindings.
//
// Class/method surface mirrors the reference's nanobind module signature for
// signature (reference src/starway/_bindings.pyi is the contract), with one
// extension: buffers may be host arrays (buffer protocol) OR device tensors
// (__cuda_array_interface__, e.g. torch HIP tensors) — the reference was
// CPU-only (nb::device::cpu, main.hpp:155) and left GPU "planned".
#include "buffer_parse.hpp"

#include <pybind11/functional.h>
#include <pybind11/stl.h>

namespace sw {

void bind_hooks(py::module_& m);  // module_hooks.cpp

template <Engine::Mode M>
struct PyEndpoint {
  Engine engine{M};
  explicit PyEndpoint(Context&) {
    engine.preferred_device_ = gpu::current_device();
  }
};
using PyServer = PyEndpoint<Engine::ServerMode>;
using PyClient = PyEndpoint<Engine::ClientMode>;

// send of both endpoint classes; ep is null for a client.
static void send_message(Engine& engine, std::shared_ptr<EndpointInfo> ep,
                         py::object buffer, uint64_t tag, py::object done,
                         py::object fail, py::object index) {
  BufferRef ref = parse_message_buffer(buffer, std::move(index),
                                       /*writable=*/false);
  engine.send(std::move(ep), ref, tag, std::move(done), std::move(fail),
              std::move(buffer));
}

// get_stats() of both endpoint classes: the keys in this order.
static py::dict stats_dict(const Engine::Stats& st) {
  py::dict d;
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
  d["cast_rx"] = st.cast_rx.load();
  d["index_tx"] = st.index_tx.load();
  d["index_rx"] = st.index_rx.load();
  return d;
}

// What Server and Client bind alike.
template <class T>
static void bind_common(py::class_<T>& cls) {
  cls.def("get_worker_address",
          [](T& e) {
            auto v = e.engine.get_worker_address();
            return py::bytes((const char*)v.data(), v.size());
          })
      .def("close", [](T& e, py::object cb) { e.engine.close(std::move(cb)); },
           py::arg("callback"))
      .def("recv",
           [](T& e, py::object buffer, uint64_t tag, uint64_t tag_mask,
              py::object done, py::object fail, const std::string& reduce,
              const std::string& dtype, py::object index,
              const std::string& msg_dtype) {
             BufferRef ref = parse_message_buffer(
                 buffer, std::move(index), /*writable=*/true, reduce, dtype,
                 msg_dtype);
             e.engine.recv(ref, tag, tag_mask, std::move(done),
                           std::move(fail), std::move(buffer));
           },
           py::arg("buffer"), py::arg("tag"), py::arg("tag_mask"),
           py::arg("done_callback"), py::arg("fail_callback"),
           py::arg("reduce") = "", py::arg("dtype") = "",
           py::arg("index") = py::none(), py::arg("msg_dtype") = "")
      .def("flush",
           [](T& e, py::object done, py::object fail) {
             e.engine.flush(std::move(done), std::move(fail));
           },
           py::arg("done_callback"), py::arg("fail_callback"))
      .def("get_stats", [](T& e) { return stats_dict(e.engine.stats_); });
}

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

  py::class_<PyServer> server(m, "Server");
  bind_common(server);
  server
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
      .def("send",
           [](PyServer& s, std::shared_ptr<EndpointInfo> ep, py::object buffer,
              uint64_t tag, py::object done, py::object fail,
              py::object index) {
             send_message(s.engine, std::move(ep), std::move(buffer), tag,
                          std::move(done), std::move(fail), std::move(index));
           },
           py::arg("client_ep"), py::arg("buffer"), py::arg("tag"),
           py::arg("done_callback"), py::arg("fail_callback"),
           py::arg("index") = py::none())
      .def("flush_ep",
           [](PyServer& s, std::shared_ptr<EndpointInfo> ep, py::object done,
              py::object fail) {
             s.engine.flush_ep(std::move(ep), std::move(done),
                               std::move(fail));
           },
           py::arg("client_ep"), py::arg("done_callback"),
           py::arg("fail_callback"))
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

  py::class_<PyClient> client(m, "Client");
  bind_common(client);
  client
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
      .def("send",
           [](PyClient& c, py::object buffer, uint64_t tag, py::object done,
              py::object fail, py::object index) {
             send_message(c.engine, nullptr, std::move(buffer), tag,
                          std::move(done), std::move(fail), std::move(index));
           },
           py::arg("buffer"), py::arg("tag"), py::arg("done_callback"),
           py::arg("fail_callback"), py::arg("index") = py::none())
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
  bind_hooks(m);
  m.attr("__version__") = "0.1.0";
}
