// starway_amd engine, matching: posted/unexpected queues, doorbell
// conflict resolution at match time, flush progress.

#include "engine_internal.hpp"

namespace sw {

// ---- recv matching --------------------------------------------------------

// STARWAY_UNEXP_CAP: per-connection unexpected-staging receive window
// (0 disables). Chosen well above the test suite's 32 MiB staging cases
// but far below RAM scale.
uint64_t unexp_cap() {
  static const uint64_t cap = env_u64("STARWAY_UNEXP_CAP", 512ull << 20);
  return cap;
}

std::string truncated_msg(uint64_t len, uint64_t cap) {
  return "message truncated (len " + std::to_string(len) + " > buffer " +
         std::to_string(cap) + ")";
}

std::string reduce_len_msg(uint64_t len, const BufferRef& buf) {
  if (buf.converting())
    return "msg_dtype: message length " + std::to_string(len) +
           " B is not a multiple of the message's item size (" +
           std::to_string(elem_size(buf.msg_elem)) + " B)";
  return "reduce: message length " + std::to_string(len) +
         " B is not a multiple of the item size (" +
         std::to_string(elem_size(buf.elem)) + " B)";
}

void Engine::unstage_unexp(UnexpectedMsg* um) {
  if (!um->staged) return;
  if (um->conn) um->conn->unexp_staged_bytes -= um->staged;
  stats_.unexp_staged_bytes.fetch_sub(um->staged, std::memory_order_relaxed);
  um->staged = 0;
}

// Resolve a doorbell conflict: another delivery path selected the armed
// recv. Cancel the wait kernel and see who won. Returns true when the recv
// is still available; false when the kernel consumed a message into it
// first (armed_done_ records the copy until its SMSG frame arrives).
bool Engine::steal_armed(Op* r) {
  gpu::arm_cancel(armed_.ticket);
  uint64_t sz = 0;
  int st = 0;
  wait_while(std::chrono::milliseconds(100), [&] {
    return (st = gpu::arm_poll(armed_.ticket, &sz)) == 0;
  });
  bool copied = (st == 1);
  retire_armed_ticket(armed_.ticket);
  Connection* conn = armed_.conn;
  uint64_t seq = armed_.seq;
  armed_ = Armed{};
  if (!copied) return true;
  // The kernel copied message `seq` into r before we could cancel: r is
  // spoken for; complete it when the control frame (with the tag) lands.
  unpost_recv(r);
  armed_done_ = ArmedDone{true, conn, seq, sz, r};
  return false;
}

bool Engine::unpost_recv(Op* r) {
  for (auto it = posted_recvs_.begin(); it != posted_recvs_.end(); ++it) {
    if (*it == r) {
      posted_recvs_.erase(it);
      return true;
    }
  }
  return false;
}

// Find and REMOVE the first posted recv matching `tag`, resolving doorbell
// conflicts. Every delivery path matches through here so the doorbell can
// never race a completion.
Op* Engine::take_matching_recv(uint64_t tag) {
restart:
  for (auto it = posted_recvs_.begin(); it != posted_recvs_.end(); ++it) {
    Op* r = *it;
    if ((tag & r->tag_mask) != (r->tag & r->tag_mask)) continue;
    if (armed_.ticket && armed_.recv_op == r) {
      if (!steal_armed(r)) goto restart;  // doorbell consumed r: rescan
      // steal_armed left r posted; the iterator may be stale — rescan.
      if (unpost_recv(r)) return r;
      goto restart;
    }
    posted_recvs_.erase(it);
    return r;
  }
  return nullptr;
}

void Engine::repost_recv_front(Op* r) {
  if (armed_.ticket) {
    // The front of the posted queue is changing: the armed recv is no
    // longer the first match candidate, so the doorbell must stand down.
    Op* armed_r = armed_.recv_op;
    if (!steal_armed(armed_r)) {
      // It consumed a message meanwhile; armed_done_ tracks it.
    }
  }
  posted_recvs_.push_front(r);
}

void Engine::match_or_stash_recv(Op* op) {
  arm_streak_ = 0;
  arm_backoff_ = false;  // fresh recv: the doorbell may re-engage
  if (!try_match_unexpected(op)) posted_recvs_.push_back(op);
}

bool Engine::try_match_unexpected(Op* op) {
  for (auto it = unexpected_.begin(); it != unexpected_.end(); ++it) {
    UnexpectedMsg* um = it->get();
    if (um->bound_recv) continue;
    if ((um->tag & op->tag_mask) != (op->tag & op->tag_mask)) continue;
    // Only an eager message can still be streaming in (descriptors are
    // parked complete); it stays queued until its last byte arrives.
    if (!um->complete) {
      um->bound_recv = op;  // delivered when the stream finishes
      if (op->buf.device < 0 && um->size <= op->buf.size) {
        // Redirect: staged prefix now, remainder streams zero-copy.
        memcpy(op->buf.ptr, um->data.data(), um->got);
        um->redirect_dst = op->buf.ptr;
        um->data.clear();
        unstage_unexp(um);
      }
      return true;
    }
    // Out of the queue before anything below can re-enter it.
    std::unique_ptr<UnexpectedMsg> msg = std::move(*it);
    unexpected_.erase(it);
    if (msg->is_rts)
      start_gpu_pull(op, msg->rts, msg->rts_index, msg->tag, msg->size,
                     msg->sender_op_id, msg->conn);
    else if (msg->is_cma)
      start_cma_pull(op, msg->cma, msg->tag, msg->size, msg->sender_op_id,
                     msg->conn);
    else if (msg->is_smsg)
      dispatch_smsg_to_recv(msg->conn, op, msg->tag, msg->size,
                            msg->smsg_seq);
    else
      complete_recv_from_unexpected(op, msg.release());
    return true;
  }
  return false;
}

// Queue a message no posted recv matched and whose descriptor is complete
// (RTS / CMA / inbox); the caller fills in the plane-specific part.
UnexpectedMsg* Engine::park_unexpected(Connection* c, uint64_t tag,
                                       uint64_t size, uint64_t sender_op) {
  auto um = std::make_unique<UnexpectedMsg>();
  um->tag = tag;
  um->size = size;
  um->conn = c;
  um->sender_op_id = sender_op;
  um->complete = true;
  unexpected_.push_back(std::move(um));
  return unexpected_.back().get();
}

void Engine::complete_recv_from_unexpected(Op* op, UnexpectedMsg* um) {
  std::unique_ptr<UnexpectedMsg> guard(um);
  unstage_unexp(um);
  if (um->redirect_dst) {
    // Stream was redirected into the recv buffer; payload already in place.
    // This delivery has never bumped a counter, unlike every other one
    // (known asymmetry, kept as is): hence the counter-less plane.
    deliver_recv(op, um->tag, um->size, RxPlane::None);
    return;
  }
  if (!op->buf.accepts(um->size)) {
    fail_op(op, "receive failed: " +
                    truncated_msg(um->size, op->buf.capacity()));
    return;
  }
  if (!op->buf.whole_elems(um->size)) {
    fail_op(op, "receive failed: " + reduce_len_msg(um->size, op->buf));
    return;
  }
  if (op->buf.device >= 0) {
    upload_to_recv(op, um->tag, um->size, std::move(um->data));
    return;
  }
  memcpy(op->buf.ptr, um->data.data(), um->size);
  deliver_recv(op, um->tag, um->size, RxPlane::Eager);
}

// ---- flush ----------------------------------------------------------------

void Engine::check_flush_progress() {
  for (Op* f : pending_flushes_) {
    for (auto it = f->flush_write_targets.begin();
         it != f->flush_write_targets.end();) {
      if (it->first->tx_written_bytes >= it->second)
        it = f->flush_write_targets.erase(it);
      else
        ++it;
    }
  }
  complete_drained_flushes();
}

// Complete every pending flush with nothing left to wait for.
void Engine::complete_drained_flushes() {
  for (size_t i = 0; i < pending_flushes_.size();) {
    Op* f = pending_flushes_[i];
    if (f->flush_write_targets.empty() && f->flush_ops_pending.empty()) {
      complete_flush(f);
      pending_flushes_.erase(pending_flushes_.begin() + i);
    } else {
      i++;
    }
  }
}

void Engine::forget_send_in_flushes(uint64_t op_id) {
  for (Op* f : pending_flushes_) f->flush_ops_pending.erase(op_id);
}

// Drop `ids` from one flush's pending sends; true when it covered any.
bool flush_forgets_any(Op* f, const std::vector<uint64_t>& ids) {
  bool hit = false;
  for (uint64_t id : ids)
    if (f->flush_ops_pending.erase(id)) hit = true;
  return hit;
}

// Fail (and drop) every pending flush pred selects. pred may also prune
// the flush's own bookkeeping as it looks.
void Engine::fail_flushes_where(const std::function<bool(Op*)>& pred,
                                const std::string& reason) {
  for (size_t i = 0; i < pending_flushes_.size();) {
    Op* f = pending_flushes_[i];
    if (pred(f)) {
      fail_op(f, reason);
      pending_flushes_.erase(pending_flushes_.begin() + i);
    } else {
      i++;
    }
  }
}

}  // namespace sw
