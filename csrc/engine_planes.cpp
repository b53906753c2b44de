// starway_amd engine, message planes: GPU RTS pull (+ batching), CMA
// pull, cross-host d2h, the small-message inbox and its doorbell.

#include "engine_internal.hpp"

#include <errno.h>
#include <sys/uio.h>

namespace sw {

static bool debug_arm() {
  static const bool on = getenv("STARWAY_DEBUG_ARM") != nullptr;
  return on;
}

// ---- GPU rendezvous -------------------------------------------------------

void Engine::handle_rts(Connection* c, const RtsDesc& rts,
                        const IndexRef& src_index, uint64_t tag, uint64_t size,
                        uint64_t sender_op) {
  if (Op* r = take_matching_recv(tag)) {
    start_gpu_pull(r, rts, src_index, tag, size, sender_op, c);
    return;
  }
  // A parked descriptor keeps its index list until the receive is posted.
  UnexpectedMsg* um = park_unexpected(c, tag, size, sender_op);
  um->is_rts = true;
  um->rts = rts;
  um->rts_index = src_index;
}

void Engine::start_gpu_pull(Op* recv_op, const RtsDesc& rts,
                            const IndexRef& src_index, uint64_t tag,
                            uint64_t size, uint64_t sender_op, Connection* c) {
  // A rows window offered a shorter message is let through on purpose:
  // begin_pull refuses it with its geometry text, which is what callers of
  // this plane have always seen, not the truncation text.
  const BufferRef& buf = recv_op->buf;
  if (!buf.accepts(size) && !(buf.rows > 0 && size < buf.size)) {
    reject_rndv(c, sender_op, recv_op, truncated_msg(size, buf.capacity()));
    return;
  }
  if (!buf.whole_elems(size)) {
    reject_rndv(c, sender_op, recv_op, reduce_len_msg(size, buf));
    return;
  }
  // Small contiguous device->device messages are batched: collected here,
  // launched as one multi-copy kernel + one event at the end of the loop
  // iteration (the per-launch cost dominates small-message rate). Never a
  // reducing recv: k_copy_multi overwrites. Never an indexed source: its
  // descriptor alone describes the pool's base, not the message.
  static const uint64_t multi_copy_max =
      env_u64("STARWAY_MULTI_COPY_MAX", 65536);
  if (size > 0 && size <= multi_copy_max && buf.device >= 0 && buf.plain() &&
      rts.contiguous() && !src_index.on()) {
    pending_small_pulls_.push_back(
        SmallPull{rts, recv_op, c, sender_op, tag, size});
    return;
  }
  std::string err;
  void* ticket = gpu::begin_pull(rts, src_index, buf, size, &err);
  if (!ticket) {
    reject_rndv(c, sender_op, recv_op, err);
    return;
  }
  track_gpu_ticket(ticket, {SmallPull{rts, recv_op, c, sender_op, tag, size}});
}

void Engine::track_gpu_ticket(void* ticket, std::vector<SmallPull> items) {
  auto pull = std::make_unique<GpuPull>();
  pull->ticket = ticket;
  pull->items = std::move(items);
  gpu_pulls_.push_back(std::move(pull));
}

bool Engine::upload_to_recv(Op* r, uint64_t tag, uint64_t len,
                            RawBuf&& bounce, RxPlane plane) {
  std::string err;
  void* ticket = gpu::begin_h2d(r->buf, bounce.data(), len, &err);
  if (!ticket) {
    fail_op(r, "receive failed: " + err);
    return false;
  }
  // The ticket owns the bounce until the copy lands. No sender op: the
  // upload completes through poll_gpu (counted on `plane`, gpu_rx unless
  // the caller says otherwise) and acks nobody.
  gpu::attach_bounce(ticket, std::move(bounce));
  bounce.clear();
  track_gpu_ticket(ticket,
                   {SmallPull{RtsDesc{}, r, nullptr, 0, tag, len, plane}});
  return true;
}

void Engine::flush_small_pulls() {
  // Group by destination device; launch batches of up to kMultiMax per
  // kernel. A lone pull goes through the ordinary single path.
  while (!pending_small_pulls_.empty()) {
    int dev = pending_small_pulls_[0].recv_op->buf.device;
    gpu::PullReq reqs[kMultiMax];
    SmallPull items[kMultiMax];
    int n = 0;
    for (size_t i = 0; i < pending_small_pulls_.size() && n < kMultiMax;) {
      if (pending_small_pulls_[i].recv_op->buf.device == dev) {
        items[n] = pending_small_pulls_[i];
        reqs[n] = gpu::PullReq{items[n].rts, items[n].recv_op->buf.ptr, dev,
                               items[n].size};
        n++;
        pending_small_pulls_.erase(pending_small_pulls_.begin() + i);
      } else {
        i++;
      }
    }
    std::string err;
    void* ticket = nullptr;
    if (n == 1) {
      ticket = gpu::begin_pull(items[0].rts, IndexRef{},
                               items[0].recv_op->buf, items[0].size, &err);
    } else {
      ticket = gpu::begin_pull_multi(reqs, n, &err);
    }
    if (!ticket) {
      for (int i = 0; i < n; i++)
        reject_rndv(items[i].conn, items[i].sender_op_id, items[i].recv_op,
                    err);
      continue;
    }
    track_gpu_ticket(ticket, std::vector<SmallPull>(items, items + n));
  }
}

// ---- small-message inbox plane --------------------------------------------

void Engine::inbox_release_seq(Connection* c, uint64_t seq) {
  c->inbox_released.insert(seq);
  while (c->inbox_released.count(c->inbox_consumed + 1)) {
    c->inbox_released.erase(c->inbox_consumed + 1);
    c->inbox_consumed++;
  }
  if (!c->dead &&
      c->inbox_consumed - c->inbox_credited >=
          std::max<uint64_t>(1, c->inbox_l.slots / 4)) {
    enqueue_frame(c, FT_INBOX_CREDIT, 0, 0, c->inbox_consumed, nullptr, 0,
                  true);
    c->inbox_credited = c->inbox_consumed;
  }
}

// Route one announced inbox message to a matched recv: batched local
// unpack kernel (device dst) or pinned bounce (host / strided / reducing
// dst; the unpack kernel overwrites).
void Engine::dispatch_smsg_to_recv(Connection* c, Op* r, uint64_t tag,
                                   uint64_t size, uint64_t seq) {
  if (!r->buf.accepts(size)) {
    fail_op(r, "receive failed: " + truncated_msg(size, r->buf.capacity()));
    inbox_release_seq(c, seq);  // discard without reading the slot
    return;
  }
  if (!r->buf.whole_elems(size)) {
    fail_op(r, "receive failed: " + reduce_len_msg(size, r->buf));
    inbox_release_seq(c, seq);
    return;
  }
  uint8_t* dst = nullptr;
  if (r->buf.device >= 0 && r->buf.plain() &&
      r->buf.device == c->inbox_l.device)
    dst = r->buf.ptr;
  pending_unpacks_.push_back(PendingUnpack{c, seq, size, tag, r, dst});
}

void Engine::handle_smsg(Connection* c, uint64_t tag, uint64_t size,
                         uint64_t seq) {
  c->inbox_seen_seq = seq;
  arm_streak_ = 0;
  arm_backoff_ = false;
  // Doorbell copy that raced a disarm: this frame carries its tag.
  if (armed_done_.active && armed_done_.conn == c && armed_done_.seq == seq) {
    Op* r = armed_done_.recv_op;
    armed_done_ = ArmedDone{};
    deliver_recv(r, tag, size, RxPlane::Doorbell);
    inbox_release_seq(c, seq);
    try_arm();
    return;
  }
  // Doorbell fast path: a pre-armed kernel is watching exactly this seq.
  if (armed_.ticket && armed_.conn == c && armed_.seq == seq) {
    auto dbg_t0 = std::chrono::steady_clock::now();
    uint64_t sz = 0;
    int st = gpu::arm_poll(armed_.ticket, &sz);
    int st_first = st;
    auto still_running = [&] {
      return (st = gpu::arm_poll(armed_.ticket, &sz)) == 0;
    };
    if (st == 0) {
      // The payload and this control frame race each other; the kernel
      // sees the slot within microseconds of the xGMI write landing. Tight
      // spin, no yield: this is the latency path.
      wait_while(std::chrono::milliseconds(
                     (long)env_u64("STARWAY_ARM_WAIT_MS", 2)),
                 still_running, /*yield=*/false);
      if (st == 0) {
        gpu::arm_cancel(armed_.ticket);
        wait_while(std::chrono::milliseconds(100), still_running);
        // Diagnostic (STARWAY_DEBUG_ARM=1): a doorbell that had to be
        // canceled because it never reported, with its final state.
        if (debug_arm())
          fprintf(stderr, "[sw-arm] seq=%llu missed, final st=%d\n",
                  (unsigned long long)seq, st);
      }
    }
    if (debug_arm()) {
      double us = std::chrono::duration<double, std::micro>(
                      std::chrono::steady_clock::now() - dbg_t0)
                      .count();
      if (us > 100 || st != 1)
        fprintf(stderr,
                "[sw-arm] seq=%llu first_st=%d final_st=%d wait=%.0fus\n",
                (unsigned long long)seq, st_first, st, us);
    }
    Op* r = armed_.recv_op;
    retire_armed_ticket(armed_.ticket);
    armed_ = Armed{};
    if (st == 1) {
      unpost_recv(r);
      deliver_recv(r, tag, sz, RxPlane::Doorbell);
      inbox_release_seq(c, seq);
      try_arm();
      return;
    }
    // nomatch / canceled / expired / stuck: the recv stays posted and the
    // message goes through the ordinary path below.
  }
  if (Op* r = take_matching_recv(tag)) {
    dispatch_smsg_to_recv(c, r, tag, size, seq);
    return;
  }
  stats_.unexpected_rx.fetch_add(1, std::memory_order_relaxed);
  UnexpectedMsg* um = park_unexpected(c, tag, size, /*sender_op=*/0);
  um->is_smsg = true;
  um->smsg_seq = seq;
}

void Engine::flush_pending_pushes() {
  for (auto& [c, vec] : pending_pushes_) {
    if (vec.empty()) continue;
    if (c->dead) {
      for (auto& pp : vec) {
        gpu_sends_.erase(pp.op->id);
        fail_op(pp.op, "send failed: connection reset");
      }
      vec.clear();
      continue;
    }
    bool same_proc = memcmp(c->peer.uuid, process_uuid(), 16) == 0;
    size_t i = 0;
    while (i < vec.size()) {
      // One launch per (destination ring, source device) batch.
      int run_dev = vec[i].op->buf.device;
      gpu::PushMsg msgs[32];
      auto batch = std::make_unique<PushBatch>();
      batch->conn = c;
      int n = 0;
      size_t j = i;
      while (j < vec.size() && n < 32) {
        if (vec[j].op->buf.device != run_dev) {
          j++;
          continue;
        }
        msgs[n] = gpu::PushMsg{vec[j].op->buf.ptr,
                               (uint32_t)vec[j].op->buf.size, vec[j].seq,
                               vec[j].op->tag};
        batch->ops.push_back(vec[j].op);
        vec.erase(vec.begin() + j);
        n++;
      }
      std::string err;
      batch->ticket =
          gpu::inbox_push(c->inbox_r, same_proc, run_dev, msgs, n,
                          engine_lane_, &err);
      if (!batch->ticket) {
        // Push plane broken: fail these sends and stop using the inbox.
        c->inbox_r_active = false;
        for (Op* op : batch->ops) {
          gpu_sends_.erase(op->id);
          fail_op(op, "send failed: " + err);
        }
      } else {
        push_batches_.push_back(std::move(batch));
      }
    }
  }
  pending_pushes_.clear();
}

void Engine::progress_pushes(bool& did_work) {
  for (size_t i = 0; i < push_batches_.size();) {
    PushBatch* b = push_batches_[i].get();
    std::string err;
    int r = gpu::push_poll(b->ticket, &err);
    if (r == 0) {
      i++;
      continue;
    }
    did_work = true;
    gpu::push_free(b->ticket);
    for (Op* op : b->ops) {
      gpu_sends_.erase(op->id);
      if (r < 0) {
        forget_send_in_flushes(op->id);
        fail_op(op, "send failed: " + err);
      } else if (!b->conn || b->conn->dead) {
        forget_send_in_flushes(op->id);
        fail_op(op, "send failed: connection reset");
      } else {
        on_send_wire_handoff(op, b->conn);
        complete_send(op);
      }
    }
    push_batches_.erase(push_batches_.begin() + i);
  }
}

void Engine::flush_pending_unpacks() {
  while (!pending_unpacks_.empty()) {
    Connection* c = pending_unpacks_[0].conn;
    auto batch = std::make_unique<UnpackBatch>();
    batch->conn = c;
    gpu::UnpackMsg msgs[32];
    int n = 0;
    for (size_t i = 0; i < pending_unpacks_.size() && n < 32;) {
      if (pending_unpacks_[i].conn == c) {
        msgs[n] = gpu::UnpackMsg{pending_unpacks_[i].seq,
                                 (uint32_t)pending_unpacks_[i].size,
                                 pending_unpacks_[i].dst};
        batch->msgs.push_back(pending_unpacks_[i]);
        pending_unpacks_.erase(pending_unpacks_.begin() + i);
        n++;
      } else {
        i++;
      }
    }
    std::string err;
    batch->ticket =
        gpu::inbox_unpack(c->inbox_l, msgs, n, engine_lane_, &err);
    if (!batch->ticket) {
      for (auto& m : batch->msgs) {
        fail_op(m.recv_op, "receive failed: " + err);
        inbox_release_seq(c, m.seq);
      }
      continue;
    }
    batch->done.assign(batch->msgs.size(), false);
    batch->remaining = batch->msgs.size();
    unpack_batches_.push_back(std::move(batch));
  }
}

void Engine::progress_unpacks(bool& did_work) {
  for (size_t i = 0; i < unpack_batches_.size();) {
    UnpackBatch* b = unpack_batches_[i].get();
    for (size_t k = 0; k < b->msgs.size(); k++) {
      if (b->done[k]) continue;
      std::string err;
      int r = gpu::unpack_poll(b->ticket, (int)k, &err);
      if (r == 0) continue;
      did_work = true;
      b->done[k] = true;
      b->remaining--;
      PendingUnpack& m = b->msgs[k];
      if (b->probe) {
        if (r > 0 && m.conn && !m.conn->dead) {
          m.conn->inbox_consumed = m.seq;
          m.conn->inbox_credited = m.seq;
          enqueue_frame(m.conn, FT_INBOX_CREDIT, 0, 0, m.seq, nullptr, 0,
                        true);
        } else if (r < 0) {
          fprintf(stderr,
                  "[starway] inbox bring-up probe never landed — push "
                  "plane disabled for this connection (RTS fallback)\n");
        }
        continue;
      }
      if (r < 0) {
        // The in-kernel wait expired before the payload landed. Under a
        // loaded launch queue the push kernel can start tens of ms late,
        // so retry (fresh unpack kernel) before declaring the message
        // lost (sender died mid-push => recv stays pending, the
        // unflushed-close contract).
        if (m.retries + 1 < 50 && m.conn && !m.conn->dead) {
          PendingUnpack again = m;
          again.retries++;
          pending_unpacks_.push_back(again);
        } else {
          repost_recv_front(m.recv_op);
          inbox_release_seq(m.conn, m.seq);
        }
        continue;
      }
      if (!m.dst) {
        const uint8_t* bounce = gpu::unpack_bounce(b->ticket, (int)k);
        if (m.recv_op->buf.device < 0) {
          memcpy(m.recv_op->buf.ptr, bounce, m.size);
        } else {
          // Strided / other-device recv: re-upload from a heap copy via
          // the ordinary h2d machinery (rare path, <= slot capacity).
          RawBuf heap;
          if (!heap.alloc(m.size)) {
            fail_op(m.recv_op, "receive failed: bounce allocation failed");
          } else {
            memcpy(heap.data(), bounce, m.size);
            // Every inbox message for a reducing recv comes this way, and
            // counts as what it is, once, when it is delivered: inbox_rx.
            // (A plain strided / other-device recv on this path has always
            // counted as gpu_rx, and still does.)
            // A converting recv is one of those, reducing or not.
            const BufferRef& rb = m.recv_op->buf;
            upload_to_recv(m.recv_op, m.tag, m.size, std::move(heap),
                           rb.reducing() || rb.converting() ? RxPlane::Inbox
                                                            : RxPlane::Gpu);
          }
          inbox_release_seq(m.conn, m.seq);
          continue;
        }
      }
      deliver_recv(m.recv_op, m.tag, m.size, RxPlane::Inbox);
      inbox_release_seq(m.conn, m.seq);
    }
    if (b->remaining == 0) {
      gpu::unpack_free(b->ticket);
      unpack_batches_.erase(unpack_batches_.begin() + i);
    } else {
      i++;
    }
  }
}

void Engine::try_arm() {
  // Opt-in (STARWAY_DOORBELL=1): measured on MI355X the pre-armed
  // doorbell wins ~1.4 us one-way on a pre-posted recv but costs ~5 us
  // per direction in bidirectional pingpong (per-message arm launches on
  // both engines), so the batched-unpack path is the default.
  static const bool arm_on = [] {
    const char* v = getenv("STARWAY_DOORBELL");
    return v && !strcmp(v, "1");
  }();
  if (!arm_on || armed_.ticket || armed_done_.active || arm_backoff_)
    return;
  // Latency pattern only: with several recvs outstanding (throughput
  // pattern) a doorbell would serialize the batched unpack path into one
  // arm launch + inline wait per message.
  if (posted_recvs_.size() != 1) return;
  Op* r = posted_recvs_.front();
  // A reducing recv is never armed: the wait kernel overwrites.
  if (r->buf.device < 0 || !r->buf.plain() || r->buf.size == 0) return;
  // Only safe with exactly one live connection (its inbox FIFO is then the
  // only source of inbox messages that could race the doorbell).
  Connection* target = nullptr;
  int n_live = 0;
  for (auto& c : conns_) {
    if (c->dead) continue;
    n_live++;
    target = c.get();
  }
  if (n_live != 1 || !target || !target->inbox_l_active) return;
  if (r->buf.device != target->inbox_l.device) return;
  // Only worth a resident kernel when the expected message can actually
  // ride the inbox (small buffer): large recvs are served by the RTS pull
  // path and would just churn expired doorbells.
  if (r->buf.size > target->inbox_l.slot_bytes - gpu::kInboxHdrBytes) return;
  // Never skip ahead of inbox messages already being delivered.
  if (!pending_unpacks_.empty() || !unpack_batches_.empty()) return;
  for (auto& um : unexpected_)
    if (um->is_smsg && um->conn == target) return;
  std::string err;
  void* t = gpu::arm_recv(target->inbox_l, target->inbox_seen_seq + 1,
                          r->tag, r->tag_mask, r->buf.ptr, r->buf.size,
                          engine_lane_, /*spin_iters=*/0, &err);
  if (!t) {
    SW_DBG("arm failed: %s", err.c_str());
    return;
  }
  armed_ = Armed{t, r, target, target->inbox_seen_seq + 1};
}

void Engine::progress_armed(bool& did_work) {
  if (!armed_.ticket) return;
  uint64_t sz = 0;
  int st = gpu::arm_poll(armed_.ticket, &sz);
  if (st == 4) {
    // Bounded wait expired with no message: re-arm at the same sequence,
    // but only a few times in a row — continuous re-arming keeps a
    // spinning kernel resident ~100% of the time, which starves streams
    // sharing its hardware queue. After the streak the doorbell stands
    // down until traffic resumes (handle_smsg) or a recv is posted.
    did_work = true;
    gpu::arm_free(armed_.ticket);
    armed_ = Armed{};
    if (++arm_streak_ >= 3) {
      arm_backoff_ = true;
      return;
    }
    try_arm();
  }
  // 1 (copied) / 2 (nomatch) are resolved by handle_smsg when the control
  // frame lands; 0 keeps waiting.
}

void Engine::start_cma_pull(Op* recv_op, const CmaDesc& cma, uint64_t tag,
                            uint64_t size, uint64_t sender_op,
                            Connection* c) {
  if (!recv_op->buf.accepts(size)) {
    reject_rndv(c, sender_op, recv_op,
                truncated_msg(size, recv_op->buf.capacity()));
    return;
  }
  if (!recv_op->buf.whole_elems(size)) {
    reject_rndv(c, sender_op, recv_op, reduce_len_msg(size, recv_op->buf));
    return;
  }
  auto pull = std::make_unique<CmaPull>();
  if (recv_op->buf.device >= 0) {
    // The posted recv buffer lives on a GPU: process_vm_readv cannot write
    // device memory, so pull into a host bounce and upload with begin_h2d
    // at completion. If the bounce cannot be allocated, decline CMA — the
    // sender retransmits as eager, which handles device recvs natively.
    if (!pull->bounce.alloc(size)) {
      send_recv_fail(c, sender_op,
                     "cma unavailable (bounce allocation failed)");
      repost_recv_front(recv_op);
      return;
    }
  }
  pull->recv_op = recv_op;
  pull->conn = c;
  pull->sender_op_id = sender_op;
  pull->tag = tag;
  pull->size = size;
  pull->desc = cma;
  cma_pulls_.push_back(std::move(pull));
}

void Engine::progress_d2h(bool& did_work) {
  for (size_t i = 0; i < d2h_sends_.size();) {
    D2hSend* p = d2h_sends_[i].get();
    std::string err;
    int r = gpu::poll_ticket(p->ticket, &err);
    if (r == 0) {
      i++;
      continue;
    }
    did_work = true;
    Op* op = p->op;
    gpu::free_ticket(p->ticket);
    gpu_sends_.erase(op->id);
    release_window(op);
    if (r > 0 && op->conn && !op->conn->dead) {
      Connection* c = op->conn;
      // The staged payload is the op's captured snapshot: enqueue_eager
      // makes it the frame body (owned by the TxItem, no further copy).
      op->capture = std::move(p->buf);
      enqueue_eager(c, op);
      // Flushes that snapshot this op id now wait for the wire bytes; the
      // payload is captured in the frame => the send completes here.
      on_send_wire_handoff(op, c);
      complete_send(op);
    } else {
      forget_send_in_flushes(op->id);
      fail_op(op, r > 0 ? "send failed: connection reset"
                        : "send failed: " + err);
    }
    d2h_sends_.erase(d2h_sends_.begin() + i);
  }
}

// Chunked process_vm_readv pulls, interleaved with the progress loop so a
// multi-GiB pull never starves other connections; aborted when the sender
// dies (its memory is gone — the message is lost, recv re-posts, exactly
// the unflushed-close contract).
void Engine::progress_cma(bool& did_work) {
  constexpr size_t kChunk = 8 << 20;
  for (size_t i = 0; i < cma_pulls_.size();) {
    CmaPull* p = cma_pulls_[i].get();
    if (p->conn && p->conn->dead) {
      repost_recv_front(p->recv_op);  // data lost; recv stays pending
      cma_pulls_.erase(cma_pulls_.begin() + i);
      continue;
    }
    size_t want = (size_t)std::min<uint64_t>(kChunk, p->size - p->done);
    uint8_t* dst_base =
        p->bounce.size() ? p->bounce.data() : p->recv_op->buf.ptr;
    struct iovec liov {dst_base + p->done, want};
    struct iovec riov {(void*)(uintptr_t)(p->desc.addr + p->done), want};
    ssize_t n;
    static const bool force_eperm =
        getenv("STARWAY_CMA_FORCE_EPERM") != nullptr;  // test hook
    if (force_eperm) {
      errno = EPERM;
      n = -1;
    } else {
      n = process_vm_readv((pid_t)p->desc.pid, &liov, 1, &riov, 1, 0);
    }
    if (n < 0 && getenv("STARWAY_DEBUG_CMA"))
      fprintf(stderr, "[sw-cma] readv pid=%llu addr=%llx want=%zu errno=%d (%s)\n",
              (unsigned long long)p->desc.pid,
              (unsigned long long)(p->desc.addr + p->done), want, errno,
              strerror(errno));
    if (n < 0) {
      if (errno == EPERM || errno == ENOSYS) {
        // No ptrace rights to the sender (e.g. yama scope: a child cannot
        // read its parent). Tell the sender to retransmit as eager and
        // RE-POST the recv so the retransmission matches it.
        send_recv_fail(
            p->conn, p->sender_op_id,
            "cma unavailable (" + std::string(strerror(errno)) + ")");
        repost_recv_front(p->recv_op);
      } else {
        // ESRCH/EFAULT: sender died or freed the buffer mid-pull — the
        // message is lost; the recv stays pending (unflushed-close
        // contract).
        repost_recv_front(p->recv_op);
      }
      cma_pulls_.erase(cma_pulls_.begin() + i);
      continue;
    }
    did_work = true;
    p->done += (uint64_t)n;
    if (p->done >= p->size) {
      // Data is out of the sender's address space => ack now (the sender
      // may reuse/free its buffer); any device upload is local work.
      enqueue_frame(p->conn, FT_RECV_DONE, 0, p->sender_op_id, 0, nullptr, 0,
                    true);
      if (p->bounce.size()) {
        // Device recv: upload the bounce; the recv completes with the h2d
        // ticket (poll_gpu), which also owns the bounce's lifetime. The
        // pull itself still counts as cma_rx here.
        stats_.cma_rx.fetch_add(1, std::memory_order_relaxed);
        upload_to_recv(p->recv_op, p->tag, p->size, std::move(p->bounce));
      } else {
        deliver_recv(p->recv_op, p->tag, p->size, RxPlane::Cma);
      }
      cma_pulls_.erase(cma_pulls_.begin() + i);
      continue;
    }
    i++;
  }
}

void Engine::poll_gpu(bool& did_work) {
  for (size_t i = 0; i < gpu_pulls_.size();) {
    GpuPull* p = gpu_pulls_[i].get();
    std::string err;
    int r = gpu::poll_ticket(p->ticket, &err);
    if (r == 0) {
      i++;
      continue;
    }
    did_work = true;
    for (auto& it : p->items) {
      if (r > 0) {
        if (it.sender_op_id && it.conn && !it.conn->dead)
          enqueue_frame(it.conn, FT_RECV_DONE, 0, it.sender_op_id, 0, nullptr,
                        0, true);
        deliver_recv(it.recv_op, it.tag, it.size, it.plane);
      } else {
        reject_rndv(it.conn, it.sender_op_id, it.recv_op, err);
      }
    }
    gpu::free_ticket(p->ticket);
    gpu_pulls_.erase(gpu_pulls_.begin() + i);
  }
}

void Engine::on_gpu_send_acked(uint64_t op_id, bool failed,
                               const std::string& err) {
  auto it = gpu_sends_.find(op_id);
  if (it == gpu_sends_.end()) return;
  Op* op = it->second;
  gpu_sends_.erase(it);
  release_window(op);
  if (failed && op->buf.device < 0 &&
      err.find("cma unavailable") != std::string::npos && op->conn &&
      !op->conn->dead) {
    op->conn->cma_denied = true;  // stop offering CMA on this connection
    // Receiver cannot process_vm_readv us (e.g. yama ptrace restrictions):
    // retransmit the message as a plain eager stream (the captured
    // snapshot, when present, becomes the frame body). The send op already
    // completed (handed off); extend any pending flush that covered it to
    // the new write target so flush still means delivery.
    bool captured = enqueue_eager(op->conn, op);
    on_send_wire_handoff(op, op->conn);
    // Silent completion (callbacks already consumed); else the TxItem owns
    // the op and reaps it, just as silently, at write-out.
    if (captured) complete_send(op);
    return;
  }
  if (failed) {
    fail_op(op, "send failed: " + err);
  } else {
    complete_send(op);
  }
  // Unblock flushes waiting on this op. Write targets are not re-examined
  // here; check_flush_progress does that once per loop iteration.
  forget_send_in_flushes(op_id);
  complete_drained_flushes();
}

// Free an armed ticket, or park it as a zombie while its kernel could
// still write the result cell (launch-queue backlog).
void Engine::retire_armed_ticket(void* t) {
  uint64_t sz = 0;
  if (gpu::arm_poll(t, &sz) != 0)
    gpu::arm_free(t);
  else
    zombie_arms_.push_back(t);
}

void Engine::poll_zombie_arms() {
  for (size_t i = 0; i < zombie_arms_.size();) {
    uint64_t sz = 0;
    if (gpu::arm_poll(zombie_arms_[i], &sz) != 0) {
      gpu::arm_free(zombie_arms_[i]);
      zombie_arms_.erase(zombie_arms_.begin() + i);
    } else {
      i++;
    }
  }
}

}  // namespace sw
