// starway_amd engine internals shared by engine.cpp, engine_wire.cpp,
// engine_match.cpp and engine_planes.cpp. core.hpp stays the engine's
// public face (module.cpp, gpu.cpp, the stress binary); nothing outside
// the engine includes this.
#pragma once

#include "core.hpp"
#include "shm.hpp"

#include <sched.h>

#include <chrono>
#include <cstdio>
#include <string>

namespace sw {

#ifdef SW_DEBUG
#define SW_DBG(...)                      \
  do {                                   \
    fprintf(stderr, "[sw] " __VA_ARGS__); \
    fputc('\n', stderr);                 \
  } while (0)
#else
#define SW_DBG(...) \
  do {              \
  } while (0)
#endif

// Shared helpers; each is defined next to its main user.
void set_nonblocking(int fd);                         // engine_wire.cpp
const uint8_t* host_id();  // 16 bytes, stable per host; engine_wire.cpp
std::vector<std::string> local_ips();                 // engine_wire.cpp
std::vector<uint8_t> encode_worker_address(
    const std::vector<std::pair<std::string, int>>& addrs, const PeerInfo& pi);
bool decode_worker_address(const std::vector<uint8_t>& in,
                           std::vector<std::pair<std::string, int>>* addrs,
                           PeerInfo* pi);
PeerInfo self_peer_info(const std::string& name);
bool inbox_enabled();  // STARWAY_INBOX, cached at first use; engine_wire.cpp
uint64_t unexp_cap();  // STARWAY_UNEXP_CAP, cached; engine_match.cpp
std::string truncated_msg(uint64_t len, uint64_t cap);  // engine_match.cpp
// A message a reducing recv cannot take: not whole elements.
std::string reduce_len_msg(uint64_t len, const BufferRef& buf);
bool flush_forgets_any(Op* f, const std::vector<uint64_t>& ids);

// Bounded wait: polls step() while it reports "still pending", for at most
// `budget`, yielding the CPU between polls unless told not to.
template <class Step>
static void wait_while(std::chrono::milliseconds budget, Step&& step,
                       bool yield = true) {
  auto deadline = std::chrono::steady_clock::now() + budget;
  while (step()) {
    if (std::chrono::steady_clock::now() > deadline) break;
    if (yield) sched_yield();
  }
}

// ---------------------------------------------------------------------------
// GpuPull — one in-flight GPU ticket (RTS pull, batched small pulls, or a
// host->device bounce upload) and the recvs it completes
// ---------------------------------------------------------------------------

struct Engine::GpuPull {
  void* ticket = nullptr;
  // One entry per message sharing the ticket (a single pull is a batch of
  // one). Each recv completes with (tag, size); sender_op_id 0 => no
  // RECV_DONE/RECV_FAIL ack (h2d bounce), and conn is read only with a
  // nonzero sender_op_id.
  std::vector<Engine::SmallPull> items;
};

}  // namespace sw
