// starway_amd engine — progress thread, TCP plane, tag matching, GPU
// rendezvous orchestration.
//
// Design notes (API/behavior parity targets cite the reference):
//  * one progress thread per Client/Server object; all transport state is
//    thread-confined (reference src/bindings/main.cpp:234-550 invariant)
//  * status machine 0 void / 1 init / 2 running / 3 closing / 4 closed
//    (reference src/bindings/main.hpp:173-174)
//  * tag matching: recv (tag, mask) matches message m iff
//    (m.tag & mask) == (tag & mask); posted recvs FIFO, unexpected messages
//    kept in arrival order (this replaces what UCX's matching engine did for
//    the reference at ucp_tag_recv_nbx call sites, main.cpp:404/1172)
//  * CPU sends complete when handed to the transport (buffer "reusable"
//    semantics of ucp_tag_send_nbx eager); delivery is only guaranteed after
//    flush (reference flush contract, tests/test_basic.py:250-416)
//  * GPU sends are rendezvous: RTS -> receiver pulls over xGMI -> RECV_DONE;
//    completion means delivery
//  * close cancels everything still pending with an error containing
//    "cancel" (reference main.cpp:680-701 contract)

#include "engine_internal.hpp"

#include <unistd.h>

namespace sw {

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------

Engine::Engine(Mode mode) : mode_(mode) {
  static std::atomic<int> engine_counter{0};
  engine_lane_ = engine_counter.fetch_add(1, std::memory_order_relaxed);
  if (pipe(wake_fds_) == 0) {
    set_nonblocking(wake_fds_[0]);
    set_nonblocking(wake_fds_[1]);
  }
}

Engine::~Engine() {
  int st = status_.load();
  if (st >= 1 && st < 4 && thread_.joinable()) {
    // Force-close: reference dtor safety net (main.cpp:703-719).
    status_.store(3, std::memory_order_release);
    wake();
  }
  if (thread_.joinable()) {
    py::gil_scoped_release rel;
    thread_.join();
  }
  if (listen_fd_ >= 0) ::close(listen_fd_);
  if (wake_fds_[0] >= 0) ::close(wake_fds_[0]);
  if (wake_fds_[1] >= 0) ::close(wake_fds_[1]);
}

void Engine::wake() {
  if (engine_hot_.load(std::memory_order_acquire)) return;  // already spinning
  char b = 1;
  ssize_t r = ::write(wake_fds_[1], &b, 1);
  (void)r;
}

// ---- Python-thread API ----------------------------------------------------

void Engine::listen(const std::string& addr, int port) {
  if (mode_ != ServerMode) throw std::runtime_error("not a server");
  int expect = 0;
  if (!status_.compare_exchange_strong(expect, 1))
    throw std::runtime_error("server already listening or closed");
  try {
    make_listener(addr, port);
  } catch (...) {
    status_.store(0);
    throw;
  }
  thread_ = std::thread([this] { thread_main(); });
  // Reference blocks listen() until the engine is running (main.cpp:829-831).
  py::gil_scoped_release rel;
  while (status_.load(std::memory_order_acquire) < 2) sched_yield();
}

std::vector<uint8_t> Engine::listen_address() {
  if (mode_ != ServerMode) throw std::runtime_error("not a server");
  listen("0.0.0.0", 0);  // ephemeral port; address carried in the blob
  worker_mode_ = true;
  return get_worker_address();
}

std::vector<uint8_t> Engine::get_worker_address() {
  std::vector<std::pair<std::string, int>> addrs;
  if (listen_fd_ >= 0) {
    if (listen_host_ == "0.0.0.0") {
      for (auto& ip : local_ips()) addrs.emplace_back(ip, listen_port_);
    } else {
      addrs.emplace_back(listen_host_, listen_port_);
    }
  }
  return encode_worker_address(
      addrs, self_peer_info(mode_ == ServerMode ? "server" : "client"));
}

void Engine::connect(const std::string& addr, int port, py::object cb) {
  if (mode_ != ClientMode) throw std::runtime_error("not a client");
  int expect = 0;
  if (!status_.compare_exchange_strong(expect, 1))
    throw std::runtime_error("client already connected or closed");
  connect_host_ = addr;
  connect_port_ = port;
  connect_cb_ = std::move(cb);
  connect_requested_ = true;
  thread_ = std::thread([this] { thread_main(); });
}

void Engine::connect_address(const std::vector<uint8_t>& blob, py::object cb) {
  if (mode_ != ClientMode) throw std::runtime_error("not a client");
  std::vector<std::pair<std::string, int>> addrs;
  PeerInfo pi;
  if (!decode_worker_address(blob, &addrs, &pi) || addrs.empty())
    throw std::runtime_error("invalid worker address blob");
  int expect = 0;
  if (!status_.compare_exchange_strong(expect, 1))
    throw std::runtime_error("client already connected or closed");
  connect_host_ = addrs[0].first;
  connect_port_ = addrs[0].second;
  connect_candidates_ = std::move(addrs);
  connect_cb_ = std::move(cb);
  connect_requested_ = true;
  thread_ = std::thread([this] { thread_main(); });
}

void Engine::set_accept_callback(py::object cb) {
  accept_cb_ = std::move(cb);
  have_accept_cb_ = true;
}

void Engine::close(py::object cb) {
  // The mutex makes the callback assignment visible to teardown(): the
  // engine thread may observe status 3 immediately after the CAS, and must
  // not read close_cb_ until the assignment below is complete.
  std::lock_guard<std::mutex> lk(close_mu_);
  int expect = 2;
  if (!status_.compare_exchange_strong(expect, 3))
    throw std::runtime_error(
        "close() called but the endpoint is not in a running state");
  close_cb_ = std::move(cb);
  wake();
}

void Engine::send(std::shared_ptr<EndpointInfo> ep, BufferRef buf, uint64_t tag,
                  py::object done, py::object fail, py::object keepalive) {
  if (status_.load(std::memory_order_acquire) != 2)
    throw std::runtime_error("send: endpoint not connected/running");
  Op* op = new Op();
  op->id = next_op_id_.fetch_add(1);
  op->type = OpType::Send;
  op->buf = buf;
  op->tag = tag;
  op->conn = ep ? ep->conn : nullptr;  // resolved again engine-side via ep
  op->done_cb = std::move(done);
  op->fail_cb = std::move(fail);
  op->keepalive = std::move(keepalive);
  // Stash the ep so the engine resolves conn at processing time (the raw
  // conn pointer above may already be dead).
  op->ep_ref = std::move(ep);
  {
    std::lock_guard<std::mutex> lk(cmd_mu_);
    cmd_queue_.push_back(op);
  }
  cmd_pending_.store(true, std::memory_order_release);
  wake();
}

void Engine::recv(BufferRef buf, uint64_t tag, uint64_t mask, py::object done,
                  py::object fail, py::object keepalive) {
  if (status_.load(std::memory_order_acquire) != 2)
    throw std::runtime_error("recv: endpoint not connected/running");
  Op* op = new Op();
  op->id = next_op_id_.fetch_add(1);
  op->type = OpType::Recv;
  op->buf = buf;
  op->tag = tag;
  op->tag_mask = mask;
  op->done_cb = std::move(done);
  op->fail_cb = std::move(fail);
  op->keepalive = std::move(keepalive);
  {
    std::lock_guard<std::mutex> lk(cmd_mu_);
    cmd_queue_.push_back(op);
  }
  cmd_pending_.store(true, std::memory_order_release);
  wake();
}

void Engine::flush(py::object done, py::object fail) {
  if (status_.load(std::memory_order_acquire) != 2)
    throw std::runtime_error("flush: endpoint not connected/running");
  Op* op = new Op();
  op->id = next_op_id_.fetch_add(1);
  op->type = OpType::Flush;
  op->done_cb = std::move(done);
  op->fail_cb = std::move(fail);
  {
    std::lock_guard<std::mutex> lk(cmd_mu_);
    cmd_queue_.push_back(op);
  }
  cmd_pending_.store(true, std::memory_order_release);
  wake();
}

void Engine::flush_ep(std::shared_ptr<EndpointInfo> ep, py::object done,
                      py::object fail) {
  if (status_.load(std::memory_order_acquire) != 2)
    throw std::runtime_error("flush_ep: endpoint not connected/running");
  Op* op = new Op();
  op->id = next_op_id_.fetch_add(1);
  op->type = OpType::FlushEp;
  op->done_cb = std::move(done);
  op->fail_cb = std::move(fail);
  op->ep_ref = std::move(ep);
  {
    std::lock_guard<std::mutex> lk(cmd_mu_);
    cmd_queue_.push_back(op);
  }
  cmd_pending_.store(true, std::memory_order_release);
  wake();
}

std::vector<std::shared_ptr<EndpointInfo>> Engine::list_clients() {
  std::lock_guard<std::mutex> lk(ep_mu_);
  return eps_;
}

double Engine::perf_model(bool peer_gpu, bool same_proc,
                          uint64_t msg_size) const {
  // Analytic transfer-time model, the ucp_ep_evaluate_perf analog
  // (reference main.cpp:452-467), calibrated against round-1 MI355X
  // measurements (profiles/r01_sweep_summary.md): device path ~33 us base
  // latency; same-GPU delivery ~2 TB/s; cross-GPU is xGMI-link-bound
  // (~140 GB/s sustained per pair); CPU path ~80 us / ~3 GB/s (tcp) with
  // shm/CMA improving both on the same host.
  bool self_gpu = gpu::available();
  double lat, bw;
  if (self_gpu && peer_gpu) {
    // Small messages ride the inbox push plane (~20 us one-way measured,
    // scripts/latency_probe.py); large ones the RTS pull. Bandwidths come
    // from the cached copy microbenchmark (gpu::calibrate).
    lat = 20e-6;
    bw = (same_proc ? gpu::same_gpu_copy_gbps() : gpu::xgmi_link_gbps()) *
         1e9;
  } else {
    lat = 80e-6;
    bw = 3e9;
  }
  return lat + (double)msg_size / bw;
}

double Engine::evaluate_perf(std::shared_ptr<EndpointInfo> ep,
                             uint64_t msg_size) {
  if (status_.load(std::memory_order_acquire) != 2)
    throw std::runtime_error("evaluate_perf: endpoint not running");
  if (ep) return perf_model(ep->peer_has_gpu, ep->peer_same_proc, msg_size);
  int traits = client_peer_traits_.load(std::memory_order_acquire);
  bool peer_gpu = traits > 0 && (traits & 1);
  bool same_proc = traits > 0 && (traits & 2);
  return perf_model(peer_gpu, same_proc, msg_size);
}

// ---- engine thread --------------------------------------------------------

void Engine::thread_main() {
  if (mode_ == ClientMode && connect_requested_) {
    do_connect_start();
    // 4 => connect failed (callback already fired): exit without teardown.
    // 3 can appear here when close() lands right after the successful
    // connect published status 2 — fall through so teardown() runs and the
    // close callback fires.
    if (status_.load(std::memory_order_acquire) == 4) return;
  } else {
    status_.store(2, std::memory_order_release);
  }
  bool did_work = false;
  while (status_.load(std::memory_order_acquire) == 2) {
    did_work = false;
    try {
      loop_iteration(did_work);
    } catch (const std::exception& e) {
      // Never let an engine-thread exception reach std::terminate: report
      // and shut the endpoint down (pending ops get canceled in teardown).
      fprintf(stderr, "[starway] engine error: %s — closing endpoint\n",
              e.what());
      status_.store(3, std::memory_order_release);
      break;
    }
    if (did_work) {
      idle_iters_ = 0;
    } else {
      idle_iters_++;
    }
  }
  teardown();
}

void Engine::loop_iteration(bool& did_work) {
  if (cmd_pending_.load(std::memory_order_acquire)) {
    std::vector<Op*> cmds;
    drain_commands(cmds);
    for (Op* op : cmds) {
      process_command(op);
      did_work = true;
    }
  }
  // Block in poll() only when fully idle; stay hot whenever GPU events or
  // outbound bytes are pending (the ucp_worker_progress spin analog,
  // reference main.cpp:361-468).
  // Shm rings are polled (no fd): service them every iteration.
  const uint64_t ucap = unexp_cap();
  for (auto& c : conns_) {
    if (c->dead) continue;
    if (c->shm_rx && c->shm && c->shm->rx.readable() > 0 &&
        !(ucap && c->unexp_staged_bytes >= ucap))
      handle_stream(c.get(), /*from_ring=*/true, did_work);
    if (!c->dead && !c->txq.empty() && c->txq.front().via_ring)
      handle_writable(c.get(), did_work);
    // Ring EOF: peer closed (ring flag or socket EOF) and ring drained.
    if (!c->dead && c->shm_rx && c->shm &&
        (c->shm->rx.peer_closed() || c->sock_eof) &&
        c->shm->rx.readable() == 0)
      on_conn_dead(c.get());
  }
  int timeout = 0;
  bool busy = !gpu_pulls_.empty() || !cma_pulls_.empty() ||
              !d2h_sends_.empty() || !push_batches_.empty() ||
              !unpack_batches_.empty() || !pending_pushes_.empty() ||
              !pending_unpacks_.empty() || armed_done_.active;
  if (!busy)
    for (auto& c : conns_)
      if (c->want_write() ||
          (c->shm_rx && c->shm && !c->dead && c->shm->rx.readable() > 0 &&
           !(ucap && c->unexp_staged_bytes >= ucap))) {
        busy = true;
        break;
      }
  static const uint64_t kSpinIters = env_u64("STARWAY_SPIN_ITERS", 50000);
  if (!busy && idle_iters_ > kSpinIters) timeout = 1;
  if (timeout != 0) {
    engine_hot_.store(false, std::memory_order_release);
    // Re-check for commands that raced the transition (their wake() may
    // have been skipped while we were still hot).
    if (cmd_pending_.load(std::memory_order_acquire)) {
      engine_hot_.store(true, std::memory_order_release);
      timeout = 0;
    }
  }
  poll_sockets(timeout, did_work);
  engine_hot_.store(true, std::memory_order_release);
  if (!pending_small_pulls_.empty()) {
    flush_small_pulls();
    did_work = true;
  }
  if (!pending_pushes_.empty()) {
    flush_pending_pushes();
    did_work = true;
  }
  if (!pending_unpacks_.empty()) {
    flush_pending_unpacks();
    did_work = true;
  }
  if (!push_batches_.empty()) progress_pushes(did_work);
  if (!unpack_batches_.empty()) progress_unpacks(did_work);
  if (armed_.ticket) progress_armed(did_work);
  if (!zombie_arms_.empty()) poll_zombie_arms();
  try_arm();
  if (!gpu_pulls_.empty()) poll_gpu(did_work);
  if (!cma_pulls_.empty()) progress_cma(did_work);
  if (!d2h_sends_.empty()) progress_d2h(did_work);
  if (!pending_flushes_.empty()) check_flush_progress();
  if (!completions_.empty()) {
    fire_completions();
    did_work = true;
  }
}

void Engine::drain_commands(std::vector<Op*>& cmds) {
  std::lock_guard<std::mutex> lk(cmd_mu_);
  cmds.swap(cmd_queue_);
  cmd_pending_.store(false, std::memory_order_release);
}

// STARWAY_SEND_WINDOW: per-connection cap on rendezvous bytes awaiting
// RECV_DONE (GPU RTS / CMA / cross-host d2h). Sends past the window queue
// on the connection and start as acks arrive, so a fast sender cannot pile
// unbounded staging onto a slow receiver. Default 32 GiB — generous for
// 288 GB HBM3E, tight enough that a runaway sender stalls long before OOM.
static uint64_t send_window() {
  static const uint64_t w = env_u64("STARWAY_SEND_WINDOW", 32ull << 30);
  return w;
}

bool Engine::cma_eligible(const Op* op, const Connection* c) const {
  // Large same-host CPU messages go rendezvous via process_vm_readv
  // (one copy, out of band). Threshold STARWAY_CMA_THRESHOLD bytes;
  // STARWAY_CMA=0 disables.
  static const uint64_t cma_thresh = []() -> uint64_t {
    const char* v = getenv("STARWAY_CMA");
    if (v && (!strcmp(v, "0") || !strcmp(v, "false"))) return ~0ull;
    return env_u64("STARWAY_CMA_THRESHOLD", 1 << 20);
  }();
  return op->buf.device < 0 && op->buf.size >= cma_thresh &&
         !c->cma_denied && memcmp(c->peer.host_id, host_id(), 16) == 0 &&
         memcmp(c->peer.uuid, process_uuid(), 16) != 0;
}

void Engine::release_window(Op* op) {
  if (!op->gpu_send_awaiting_ack) return;
  op->gpu_send_awaiting_ack = false;
  Connection* c = op->conn;
  if (!c) return;
  c->inflight_rndv_bytes -=
      std::min<uint64_t>(c->inflight_rndv_bytes, op->buf.size);
  if (!c->dead) drain_deferred_sends(c);
}

void Engine::drain_deferred_sends(Connection* c) {
  const uint64_t window = send_window();
  while (!c->deferred_sends.empty() && !c->dead) {
    Op* op = c->deferred_sends.front();
    bool rndv = op->buf.device >= 0 || cma_eligible(op, c);
    if (rndv && window && c->inflight_rndv_bytes > 0 &&
        c->inflight_rndv_bytes + op->buf.size > window)
      return;
    c->deferred_sends.pop_front();
    start_send(op, c);
  }
}

void Engine::on_send_wire_handoff(Op* op, Connection* c) {
  // A flush that snapshotted this op id (while it was windowed/staged) now
  // waits for the wire bytes instead.
  for (Op* f : pending_flushes_) {
    if (f->flush_ops_pending.erase(op->id)) {
      uint64_t target = c->tx_enqueued_bytes;
      auto [it, ins] = f->flush_write_targets.try_emplace(c, target);
      if (!ins && it->second < target) it->second = target;
    }
  }
}

void Engine::process_command(Op* op) {
  switch (op->type) {
    case OpType::Send: {
      Connection* c = nullptr;
      if (mode_ == ClientMode) {
        c = conns_.empty() ? nullptr : conns_[0].get();
      } else {
        c = op->ep_ref ? op->ep_ref->conn : nullptr;
      }
      if (!c || c->dead) {
        fail_op(op, "send failed: endpoint closed");
        return;
      }
      op->conn = c;
      stats_.msgs_sent.fetch_add(1, std::memory_order_relaxed);
      stats_.bytes_sent.fetch_add(op->buf.size, std::memory_order_relaxed);
      // Window admission. Any send behind already-deferred ones must also
      // queue, preserving per-connection message order for tag matching.
      const uint64_t window = send_window();
      bool rndv = op->buf.device >= 0 || cma_eligible(op, c);
      if (!c->deferred_sends.empty() ||
          (rndv && window && c->inflight_rndv_bytes > 0 &&
           c->inflight_rndv_bytes + op->buf.size > window)) {
        c->deferred_sends.push_back(op);
        stats_.deferred_sends.fetch_add(1, std::memory_order_relaxed);
        return;
      }
      start_send(op, c);
      break;
    }
    case OpType::Recv:
      match_or_stash_recv(op);
      break;
    case OpType::Flush:
    case OpType::FlushEp: {
      std::vector<Connection*> targets;
      if (op->type == OpType::FlushEp) {
        Connection* c = op->ep_ref ? op->ep_ref->conn : nullptr;
        if (!c || c->dead) {
          fail_op(op, "flush_ep failed: endpoint closed");
          return;
        }
        targets.push_back(c);
      } else {
        for (auto& c : conns_)
          if (!c->dead && c->hello_received) targets.push_back(c.get());
      }
      for (Connection* c : targets) {
        if (c->tx_written_bytes < c->tx_enqueued_bytes)
          op->flush_write_targets[c] = c->tx_enqueued_bytes;
      }
      for (auto& [id, sop] : gpu_sends_) {
        if (op->type == OpType::Flush ||
            (!targets.empty() && sop->conn == targets[0]))
          op->flush_ops_pending.insert(id);
      }
      // Window-deferred sends were posted before this flush: cover them too
      // (their ids migrate to gpu_sends_ / write targets when they start).
      for (Connection* c : targets)
        for (Op* d : c->deferred_sends) op->flush_ops_pending.insert(d->id);
      if (op->flush_write_targets.empty() && op->flush_ops_pending.empty()) {
        complete_flush(op);
      } else {
        pending_flushes_.push_back(op);
      }
      break;
    }
    default:
      fail_op(op, "internal: unknown command");
  }
}

// One window-admitted send. Completion contract (reference flush tests,
// tests/test_basic.py:250-416 + UCX buffer-reuse semantics): the done
// callback means "the engine owns the payload" — either the bytes are on
// the wire, captured into engine memory, or (GPU rendezvous) delivery is
// tracked to RECV_DONE. Delivery is only guaranteed after flush.
void Engine::start_send(Op* op, Connection* c) {
  if (op->buf.index.on())
    stats_.index_tx.fetch_add(1, std::memory_order_relaxed);
  if (cma_eligible(op, c)) {
    CmaDesc desc{};
    desc.pid = (uint64_t)getpid();
    memcpy(desc.src_uuid, process_uuid(), 16);
    // Capture: snapshot the payload so the caller may overwrite its buffer
    // the moment `await asend` returns; the receiver pulls the snapshot.
    // On allocation failure fall back to zero-copy from the live buffer
    // (keepalive pins it; contents then must not change until flush).
    static const uint64_t kCaptureMax =
        env_u64("STARWAY_CAPTURE_MAX", 1ull << 30);
    if (op->buf.size <= kCaptureMax && op->capture.alloc(op->buf.size)) {
      memcpy(op->capture.data(), op->buf.ptr, op->buf.size);
      desc.addr = (uint64_t)(uintptr_t)op->capture.data();
      dead_objs_.push_back(std::move(op->keepalive));
    } else {
      // Above the capture ceiling (or under memory pressure): the
      // receiver pulls from the live buffer; the keepalive pins it and
      // the caller must not modify it before flush (documented).
      desc.addr = (uint64_t)(uintptr_t)op->buf.ptr;
    }
    enqueue_frame(c, FT_RTS_CPU, op->tag, op->id, op->buf.size, &desc,
                  sizeof(desc), /*priority=*/false);
    op->gpu_send_awaiting_ack = true;  // same ack machinery as GPU RTS
    gpu_sends_[op->id] = op;
    c->inflight_rndv_bytes += op->buf.size;
    // Eager-style completion: payload captured/pinned; delivery guaranteed
    // only by flush (waits for RECV_DONE). Both callbacks are consumed so
    // a later cancel cannot fire fail_cb on a completed op.
    {
      py::gil_scoped_acquire gil;
      try {
        if (op->done_cb.ptr()) op->done_cb();
      } catch (py::error_already_set& e) {
        e.discard_as_unraisable("starway send callback");
      }
      op->done_cb = py::object();
      op->fail_cb = py::object();
    }
    return;
  }
  static const bool force_xhost =
      getenv("STARWAY_FORCE_XHOST") != nullptr;  // test hook
  // Small-message inbox push: device payloads up to the slot capacity are
  // written straight into the peer's ring over xGMI by a batched push
  // kernel — no RTS round trip, no per-message event, no RECV_DONE. The
  // FT_SMSG control frame is enqueued HERE so per-connection message order
  // is preserved against eager/RTS traffic. The op completes when the push
  // kernel's event lands (payload captured out of the user buffer).
  if (inbox_enabled() && op->buf.device >= 0 && op->buf.dense() &&
      op->buf.size > 0 && !force_xhost && c->inbox_r_active &&
      op->buf.size <= c->inbox_r.slot_bytes - gpu::kInboxHdrBytes &&
      c->inbox_next_seq <= c->inbox_credit_base + c->inbox_r.slots) {
    uint64_t seq = c->inbox_next_seq++;
    enqueue_frame(c, FT_SMSG, op->tag, seq, op->buf.size, nullptr, 0, false);
    op->owned_by_d2h = true;  // reaped by the push machinery, not conn-death
    gpu_sends_[op->id] = op;  // flush coverage until the push ticket lands
    pending_pushes_[c].push_back(PendingPush{op, seq});
    stats_.inbox_tx.fetch_add(1, std::memory_order_relaxed);
    return;
  }
  if (op->buf.device >= 0 &&
      (force_xhost || memcmp(c->peer.host_id, host_id(), 16) != 0)) {
    // Cross-host GPU send: hipIpc cannot cross hosts — stage the payload
    // to host memory and ship it as a plain eager frame once the download
    // completes. The op completes when the d2h ticket lands (payload
    // captured in the bounce => buffer reusable), in progress_d2h.
    auto d2h = std::make_unique<D2hSend>();
    if (!d2h->buf.alloc(op->buf.size)) {
      fail_op(op, "send failed: staging allocation failed");
      return;
    }
    std::string err;
    d2h->ticket = gpu::begin_d2h(d2h->buf.data(), op->buf, &err);
    if (!d2h->ticket) {
      fail_op(op, "send failed: " + err);
      return;
    }
    d2h->op = op;
    // Track it like a GPU send so flush waits for the wire hand-off.
    gpu_sends_[op->id] = op;
    op->gpu_send_awaiting_ack = true;
    c->inflight_rndv_bytes += op->buf.size;
    op->owned_by_d2h = true;  // progress_d2h reaps; see on_conn_dead
    d2h_sends_.push_back(std::move(d2h));
    return;
  }
  if (op->buf.device >= 0) {
    // GPU rendezvous: RTS -> receiver pulls over xGMI -> RECV_DONE. The
    // send completes at RECV_DONE (delivery), so buffer reuse is safe.
    RtsDesc rts{};
    std::string err;
    if (!gpu::make_rts(op->buf, &rts, &err)) {
      fail_op(op, "send failed: " + err);
      return;
    }
    if (op->buf.index.on()) {
      const std::vector<uint8_t> payload =
          encode_rts_indexed(&rts, sizeof(rts), op->buf.index);
      enqueue_frame(c, FT_RTS_INDEXED, op->tag, op->id, op->buf.size,
                    payload.data(), payload.size(), /*priority=*/false);
    } else {
      enqueue_frame(c, FT_RTS, op->tag, op->id, op->buf.size, &rts,
                    sizeof(rts), /*priority=*/false);
    }
    op->gpu_send_awaiting_ack = true;
    gpu_sends_[op->id] = op;
    c->inflight_rndv_bytes += op->buf.size;
  } else {
    bool captured = enqueue_eager(c, op);
    on_send_wire_handoff(op, c);  // windowed op: flush id -> write target
    // Payload written or captured => complete now (eager semantics);
    // else the TxItem owns the op and completion fires at write-out.
    if (captured) complete_send(op);
  }
}

// ---- connection death -----------------------------------------------------

void Engine::on_conn_dead(Connection* c) {
  if (c->dead) return;
  c->dead = true;
  // Doorbell armed on this connection: stand down (a copy that already
  // happened has no control frame coming — the recv fails below).
  if (armed_.ticket && armed_.conn == c) {
    Op* r = armed_.recv_op;
    if (!steal_armed(r)) {
      // Copied, but the tag-bearing frame is lost with the connection.
      armed_done_ = ArmedDone{};
      fail_op(r, "receive failed: connection reset");
    }
  }
  if (armed_done_.active && armed_done_.conn == c) {
    fail_op(armed_done_.recv_op, "receive failed: connection reset");
    armed_done_ = ArmedDone{};
  }
  // Un-launched inbox pushes to this connection never left the building.
  std::vector<uint64_t> dead_send_ids;
  auto pp = pending_pushes_.find(c);
  if (pp != pending_pushes_.end()) {
    for (auto& p : pp->second) {
      dead_send_ids.push_back(p.op->id);
      gpu_sends_.erase(p.op->id);
      fail_op(p.op, "send failed: connection reset");
    }
    pending_pushes_.erase(pp);
  }
  if (c->fd >= 0) {
    ::close(c->fd);
    c->fd = -1;
  }
  // Reference behavior: the server keeps the (stale) endpoint entry in
  // list_clients after the client closes (tests/test_basic.py:43-58).
  if (c->ep) c->ep->conn = nullptr;
  // A matched recv whose message was mid-stream goes back to pending: the
  // data is lost but the recv must NOT complete (flush-semantics tests).
  if (c->rx_recv_op) {
    repost_recv_front(c->rx_recv_op);
    c->rx_recv_op = nullptr;
  }
  if (c->rx_unexp) {
    // Incomplete unexpected message: drop it.
    for (auto it = unexpected_.begin(); it != unexpected_.end(); ++it) {
      if (it->get() == c->rx_unexp) {
        if ((*it)->bound_recv) repost_recv_front((*it)->bound_recv);
        unstage_unexp(it->get());
        unexpected_.erase(it);
        break;
      }
    }
    c->rx_unexp = nullptr;
  }
  // Complete staged unexpected messages from this conn stay matchable
  // (data fully arrived before death), but stop counting against the
  // receive window of a connection that no longer reads.
  for (auto& um : unexpected_)
    if (um->conn == c) unstage_unexp(um.get());
  drop_txq(c, "send failed: connection reset");
  // Release the shm channel now (marks our tx ring closed so the peer sees
  // EOF; the creator unlinks the segment name — the peer's own mapping
  // stays valid until it unmaps).
  c->shm_rx = false;
  c->shm_tx_enq = false;
  c->shm.reset();
  // Flushes whose write target on this conn was not reached can never
  // complete: fail them.
  fail_flushes_where(
      [c](Op* f) {
        auto it = f->flush_write_targets.find(c);
        if (it == f->flush_write_targets.end()) return false;
        if (c->tx_written_bytes < it->second) return true;
        f->flush_write_targets.erase(it);  // satisfied before death
        return false;
      },
      "flush failed: connection reset");
  // GPU sends routed to this conn will never be acked. Ops owned by the
  // d2h/push staging lists are only unregistered here — their machinery
  // reaps them (double-delete hazard otherwise). Collect the op ids so
  // flushes that snapshotted them fail instead of hanging forever.
  for (auto it = gpu_sends_.begin(); it != gpu_sends_.end();) {
    if (it->second->conn == c) {
      dead_send_ids.push_back(it->first);
      it->second->gpu_send_awaiting_ack = false;  // window already dying
      if (!it->second->owned_by_d2h)
        fail_op(it->second, "send failed: connection reset");
      it = gpu_sends_.erase(it);
    } else {
      ++it;
    }
  }
  // Window-deferred sends never started: fail them too.
  for (Op* d : c->deferred_sends) {
    dead_send_ids.push_back(d->id);
    fail_op(d, "send failed: connection reset");
  }
  c->deferred_sends.clear();
  c->inflight_rndv_bytes = 0;
  if (!dead_send_ids.empty())
    fail_flushes_where(
        [&](Op* f) { return flush_forgets_any(f, dead_send_ids); },
        "flush failed: connection reset");
}

// Drop a connection's queued tx: py keepalive refs wait for the next GIL
// hold, deferred-completion owners fail (their payload never made the
// wire).
void Engine::drop_txq(Connection* c, const std::string& reason) {
  for (auto& item : c->txq) {
    if (item.has_keepalive) {
      dead_objs_.push_back(std::move(item.keepalive));
      item.has_keepalive = false;
    }
    if (item.owner) {
      fail_op(item.owner, reason);
      item.owner = nullptr;
    }
  }
  c->txq.clear();
  c->tx_front_written = 0;
}

// ---- completion plumbing --------------------------------------------------

void Engine::complete(Completion&& comp) {
  completions_.push_back(std::move(comp));
}

void Engine::fail_op(Op* op, const std::string& reason) {
  Completion comp;
  comp.kind = Completion::Kind::Fail;
  comp.op = op;
  comp.error = reason;
  complete(std::move(comp));
}

// The one place a recv completes successfully: counts the message once
// (msgs/bytes_received + the plane's counter) and queues the callback.
// RxPlane::None counts nothing — only the mid-stream redirect uses it.
void Engine::deliver_recv(Op* r, uint64_t tag, uint64_t len, RxPlane plane) {
  if (plane != RxPlane::None) {
    stats_.msgs_received.fetch_add(1, std::memory_order_relaxed);
    stats_.bytes_received.fetch_add(len, std::memory_order_relaxed);
  }
  switch (plane) {
    case RxPlane::None:
      break;
    case RxPlane::Eager:
      stats_.eager_rx.fetch_add(1, std::memory_order_relaxed);
      break;
    case RxPlane::Gpu:
      stats_.gpu_rx.fetch_add(1, std::memory_order_relaxed);
      break;
    case RxPlane::Cma:
      stats_.cma_rx.fetch_add(1, std::memory_order_relaxed);
      break;
    case RxPlane::Doorbell:  // a doorbell delivery is also an inbox one
      stats_.doorbell_rx.fetch_add(1, std::memory_order_relaxed);
      [[fallthrough]];
    case RxPlane::Inbox:
      stats_.inbox_rx.fetch_add(1, std::memory_order_relaxed);
      break;
  }
  if (r->buf.reducing())
    stats_.reduce_rx.fetch_add(1, std::memory_order_relaxed);
  if (r->buf.converting())
    stats_.cast_rx.fetch_add(1, std::memory_order_relaxed);
  if (r->buf.index.on() && plane != RxPlane::None)
    stats_.index_rx.fetch_add(1, std::memory_order_relaxed);
  Completion comp;
  comp.kind = Completion::Kind::RecvDone;
  comp.op = r;
  comp.a = tag;
  comp.b = len;
  complete(std::move(comp));
}

void Engine::complete_send(Op* op) {
  Completion comp;
  comp.kind = Completion::Kind::SendDone;
  comp.op = op;
  complete(std::move(comp));
}

void Engine::complete_flush(Op* f) {
  Completion comp;
  comp.kind = Completion::Kind::FlushDone;
  comp.op = f;
  complete(std::move(comp));
}

void Engine::send_recv_fail(Connection* c, uint64_t sender_op,
                            const std::string& err) {
  if (sender_op && c && !c->dead)
    enqueue_frame(c, FT_RECV_FAIL, 0, sender_op, 0, err.data(), err.size(),
                  true);
}

void Engine::reject_rndv(Connection* c, uint64_t sender_op, Op* recv,
                         const std::string& err) {
  send_recv_fail(c, sender_op, err);
  fail_op(recv, "receive failed: " + err);
}

void Engine::fire_completions() {
  if (completions_.empty() && dead_objs_.empty()) return;
  std::vector<Completion> comps;
  comps.swap(completions_);
  std::vector<py::object> dead;
  dead.swap(dead_objs_);
  py::gil_scoped_acquire gil;
  dead.clear();
  for (auto& comp : comps) {
    try {
      switch (comp.kind) {
        case Completion::Kind::SendDone:
        case Completion::Kind::FlushDone:
          if (comp.op->done_cb.ptr()) comp.op->done_cb();
          break;
        case Completion::Kind::RecvDone:
          if (comp.op->done_cb.ptr()) comp.op->done_cb(comp.a, comp.b);
          break;
        case Completion::Kind::Fail:
          if (comp.op && comp.op->fail_cb.ptr()) comp.op->fail_cb(comp.error);
          break;
        case Completion::Kind::Accept:
          if (accept_cb_.ptr()) accept_cb_(comp.ep);
          break;
        case Completion::Kind::Close:
          if (comp.cb0.ptr()) comp.cb0();
          break;
        default:
          break;
      }
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("starway callback");
    }
    delete comp.op;  // py members freed under this GIL hold
    comp.op = nullptr;
    comp.cb0 = py::object();
    comp.ep.reset();
  }
}

// ---- teardown -------------------------------------------------------------

void Engine::teardown() {
  // 1. Fail everything still queued from Python threads.
  {
    std::vector<Op*> cmds;
    drain_commands(cmds);
    for (Op* op : cmds) fail_op(op, "operation canceled (endpoint closing)");
  }
  // 1b. Small-message inbox wind-down: stand the doorbell down, launch any
  //     pending pushes (their ops have not completed; they are canceled
  //     below if their kernel cannot finish), and let in-flight push/unpack
  //     kernels drain (bounded; they are microsecond-scale copies).
  if (armed_.ticket) {
    Op* r = armed_.recv_op;
    steal_armed(r);
    // If the doorbell copied at the last instant, armed_done_ now owns the
    // recv (erased from posted_recvs_) and is canceled just below; else r
    // stays posted and step 4 cancels it.
  }
  if (armed_done_.active) {
    fail_op(armed_done_.recv_op, "operation canceled (endpoint closing)");
    armed_done_ = ArmedDone{};
  }
  wait_while(std::chrono::seconds(2), [&] {
    if (!zombie_arms_.empty()) poll_zombie_arms();
    return !zombie_arms_.empty();
  });
  for (void* t : zombie_arms_) gpu::arm_leak(t);
  zombie_arms_.clear();
  for (auto& m : pending_unpacks_)
    fail_op(m.recv_op, "operation canceled (endpoint closing)");
  pending_unpacks_.clear();
  if (!pending_pushes_.empty()) flush_pending_pushes();
  {
    wait_while(std::chrono::seconds(5), [&] {
      bool did = false;
      progress_pushes(did);
      progress_unpacks(did);
      return !push_batches_.empty() || !unpack_batches_.empty();
    });
    for (auto& b : push_batches_) {
      gpu::push_free(b->ticket);
      for (Op* op : b->ops) {
        gpu_sends_.erase(op->id);
        fail_op(op, "operation canceled (endpoint closing)");
      }
    }
    push_batches_.clear();
    for (auto& b : unpack_batches_) {
      gpu::unpack_free(b->ticket);
      for (size_t k = 0; k < b->msgs.size(); k++)
        if (!b->done[k])
          fail_op(b->msgs[k].recv_op,
                  "operation canceled (endpoint closing)");
    }
    unpack_batches_.clear();
  }
  // 2. Launch any still-pending batched pulls, then let in-flight GPU
  //    pulls finish (bounded; they are plain copies), complete them and
  //    best-effort ack.
  if (!pending_small_pulls_.empty()) flush_small_pulls();
  wait_while(std::chrono::seconds(10), [&] {
    bool did = false;
    poll_gpu(did);
    return !gpu_pulls_.empty();
  });
  for (auto& p : gpu_pulls_) {
    for (auto& it : p->items)
      fail_op(it.recv_op, "operation canceled (endpoint closing)");
    gpu::free_ticket(p->ticket);
  }
  gpu_pulls_.clear();
  for (auto& p : cma_pulls_)
    fail_op(p->recv_op, "operation canceled (endpoint closing)");
  cma_pulls_.clear();
  // The async D2H copies write into the staging RawBufs below — wait for
  // their tickets (bounded) before freeing them.
  wait_while(std::chrono::seconds(10), [&] {
    bool pending = false;
    for (auto& p : d2h_sends_) {
      std::string err;
      if (gpu::poll_ticket(p->ticket, &err) == 0) pending = true;
    }
    return pending;
  });
  for (auto& p : d2h_sends_) {
    gpu::free_ticket(p->ticket);
    gpu_sends_.erase(p->op->id);
    // Never completed (completion now waits for the d2h ticket) and the
    // endpoint is closing before the payload reached the wire: cancel.
    fail_op(p->op, "operation canceled (endpoint closing)");
  }
  d2h_sends_.clear();
  // 3. Cancel in-flight data: a connection with undelivered EAGER/RTS bytes
  //    queued is closed abortively — close without flush loses in-flight
  //    sends (the reference's delivery contract, tests/test_basic.py:250-278;
  //    UCX analog: ucp_request_cancel on posted sends). This also returns any
  //    mid-stream matched recv to the posted list so the next step cancels
  //    it. Connections with only control frames left get a BYE and a short
  //    drain below so peers see a clean shutdown.
  for (auto& c : conns_) {
    if (c->dead) continue;
    bool has_data = c->tx_front_written > 0 && !c->txq.empty() &&
                    c->txq.front().is_data;
    for (auto& item : c->txq)
      if (item.is_data) has_data = true;
    if (has_data) {
      on_conn_dead(c.get());
    } else {
      enqueue_frame(c.get(), FT_BYE, 0, 0, 0, nullptr, 0, false);
    }
  }
  // 4. Cancel pending recvs / flushes / unacked GPU sends
  //    (reference cancel contract: error string contains "cancel",
  //    main.cpp:680-701, tests/test_basic.py:638-663).
  for (Op* r : posted_recvs_) fail_op(r, "operation canceled (endpoint closing)");
  posted_recvs_.clear();
  for (auto& um : unexpected_) {
    unstage_unexp(um.get());
    if (um->bound_recv)
      fail_op(um->bound_recv, "operation canceled (endpoint closing)");
  }
  unexpected_.clear();
  for (auto& c : conns_) {
    for (Op* d : c->deferred_sends)
      fail_op(d, "operation canceled (endpoint closing)");
    c->deferred_sends.clear();
  }
  for (Op* f : pending_flushes_) fail_op(f, "operation canceled (endpoint closing)");
  pending_flushes_.clear();
  for (auto& [id, op] : gpu_sends_)
    fail_op(op, "operation canceled (endpoint closing)");
  gpu_sends_.clear();
  // 5. Best-effort drain of remaining control bytes (acks, BYE) ~200 ms.
  auto deadline =
      std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
  while (std::chrono::steady_clock::now() < deadline) {
    bool any = false;
    for (auto& c : conns_) {
      if (c->dead) continue;
      if (!c->txq.empty() && c->txq.front().via_ring) {
        bool did = false;
        handle_writable(c.get(), did);
      }
      if (c->want_write()) any = true;
    }
    if (!any) break;
    bool did = false;
    poll_sockets(5, did);
  }
  for (auto& c : conns_) {
    if (c->fd >= 0) {
      ::close(c->fd);
      c->fd = -1;
    }
    if (c->ep) c->ep->conn = nullptr;
    drop_txq(c.get(), "operation canceled (endpoint closing)");
    c->shm_rx = false;
    c->shm.reset();
    if (c->inbox_l_active) {
      // Freed only after the close drain: a peer's in-flight push kernel
      // finishes in microseconds, and no new pushes can start once the
      // connection is down.
      gpu::inbox_destroy(c->inbox_l);
      c->inbox_l_active = false;
    }
  }
  if (listen_fd_ >= 0) {
    ::close(listen_fd_);
    listen_fd_ = -1;
  }
  // 6. Fire all cancellations, then the close callback, then status 4
  //    (ordering contract of reference main.cpp:469-549).
  {
    std::lock_guard<std::mutex> lk(close_mu_);
    if (close_cb_.ptr()) {
      Completion comp;
      comp.kind = Completion::Kind::Close;
      comp.cb0 = std::move(close_cb_);
      complete(std::move(comp));
    }
  }
  fire_completions();
  {
    py::gil_scoped_acquire gil;
    accept_cb_ = py::object();
    close_cb_ = py::object();
    connect_cb_ = py::object();
  }
  status_.store(4, std::memory_order_release);
}

}  // namespace sw
