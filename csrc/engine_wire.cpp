// starway_amd engine, wire plane: address/peer-info encoding, connect/
// accept, the socket loop, stream + frame parsing, the shm hand-over,
// eager rx and tx.

#include "engine_internal.hpp"

#include <errno.h>
#include <fcntl.h>
#include <ifaddrs.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <unistd.h>

#include <random>

namespace sw {

// ---------------------------------------------------------------------------
// small utils
// ---------------------------------------------------------------------------

// Env knobs with one accessor each. Read time is part of the contract:
// STARWAY_SHM is read at every use (tests flip it inside a running
// process); the others are read at first use and cached.
static bool shm_enabled() {
  const char* v = getenv("STARWAY_SHM");
  return !(v && (!strcmp(v, "0") || !strcmp(v, "false")));
}

bool inbox_enabled() {
  static const bool on = [] {
    const char* v = getenv("STARWAY_INBOX");
    return !(v && !strcmp(v, "0"));
  }();
  return on;
}

void set_nonblocking(int fd) {
  int fl = fcntl(fd, F_GETFL, 0);
  fcntl(fd, F_SETFL, fl | O_NONBLOCK);
}

static void set_tcp_opts(int fd) {
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
  static int buf = (int)env_u64("STARWAY_SOCKBUF", 8 << 20);
  setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &buf, sizeof(buf));
  setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &buf, sizeof(buf));
}

// Stable per-host identifier: FNV-1a over boot_id + hostname, 16 bytes.
const uint8_t* host_id() {
  static uint8_t id[16] = {0};
  static bool init = [] {
    std::string seed;
    FILE* f = fopen("/proc/sys/kernel/random/boot_id", "r");
    if (f) {
      char buf[128];
      size_t n = fread(buf, 1, sizeof(buf), f);
      seed.append(buf, n);
      fclose(f);
    }
    char hn[256] = {0};
    gethostname(hn, sizeof(hn) - 1);
    seed += hn;
    uint64_t h1 = 1469598103934665603ull, h2 = 14695981039346656037ull;
    for (unsigned char ch : seed) {
      h1 = (h1 ^ ch) * 1099511628211ull;
      h2 = (h2 ^ (ch + 17)) * 1099511628211ull;
    }
    memcpy(id, &h1, 8);
    memcpy(id + 8, &h2, 8);
    return true;
  }();
  (void)init;
  return id;
}

const uint8_t* process_uuid() {
  static uint8_t uuid[16] = {0};
  static bool init = [] {
    std::random_device rd;
    std::mt19937_64 gen(rd() ^ (uint64_t)getpid());
    for (int i = 0; i < 16; i += 8) {
      uint64_t v = gen();
      memcpy(uuid + i, &v, 8);
    }
    return true;
  }();
  (void)init;
  return uuid;
}

std::vector<uint8_t> encode_peer_info(const PeerInfo& pi) {
  std::vector<uint8_t> out;
  auto put = [&](const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    out.insert(out.end(), b, b + n);
  };
  uint32_t ver = kProtoVersion;
  put(&ver, 4);
  put(&pi.pid, 8);
  put(pi.uuid, 16);
  put(pi.host_id, 16);
  uint8_t hg = pi.has_gpu ? 1 : 0;
  put(&hg, 1);
  put(&pi.gpu_count, 4);
  uint16_t nl = (uint16_t)pi.name.size();
  put(&nl, 2);
  put(pi.name.data(), nl);
  return out;
}

bool decode_peer_info(const uint8_t* d, size_t len, PeerInfo* out) {
  if (len < 4 + 8 + 16 + 16 + 1 + 4 + 2) return false;
  size_t off = 0;
  uint32_t ver;
  memcpy(&ver, d + off, 4);
  off += 4;
  if (ver != kProtoVersion) return false;
  memcpy(&out->pid, d + off, 8);
  off += 8;
  memcpy(out->uuid, d + off, 16);
  off += 16;
  memcpy(out->host_id, d + off, 16);
  off += 16;
  out->has_gpu = d[off++] != 0;
  memcpy(&out->gpu_count, d + off, 4);
  off += 4;
  uint16_t nl;
  memcpy(&nl, d + off, 2);
  off += 2;
  if (off + nl > len) return false;
  out->name.assign((const char*)d + off, nl);
  return true;
}

// Worker-address blob:
//   "SWADDR1\0" | u16 n_addrs | n x { u8 iplen, ip bytes, u16 port } |
//   u32 peer_len | PeerInfo blob
static constexpr char kAddrMagic[8] = {'S', 'W', 'A', 'D', 'D', 'R', '1', 0};

std::vector<std::string> local_ips() {
  std::vector<std::string> ips;
  struct ifaddrs* ifs = nullptr;
  if (getifaddrs(&ifs) == 0) {
    for (struct ifaddrs* it = ifs; it; it = it->ifa_next) {
      if (!it->ifa_addr || it->ifa_addr->sa_family != AF_INET) continue;
      char buf[INET_ADDRSTRLEN];
      auto* sin = (struct sockaddr_in*)it->ifa_addr;
      inet_ntop(AF_INET, &sin->sin_addr, buf, sizeof(buf));
      std::string ip(buf);
      if (ip == "127.0.0.1")
        ips.push_back(ip);  // keep, but non-loopback preferred first
      else
        ips.insert(ips.begin(), ip);
    }
    freeifaddrs(ifs);
  }
  if (ips.empty()) ips.push_back("127.0.0.1");
  return ips;
}

std::vector<uint8_t> encode_worker_address(
    const std::vector<std::pair<std::string, int>>& addrs, const PeerInfo& pi) {
  std::vector<uint8_t> out(kAddrMagic, kAddrMagic + 8);
  auto put = [&](const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    out.insert(out.end(), b, b + n);
  };
  uint16_t n = (uint16_t)addrs.size();
  put(&n, 2);
  for (auto& [ip, port] : addrs) {
    uint8_t il = (uint8_t)ip.size();
    put(&il, 1);
    put(ip.data(), il);
    uint16_t p = (uint16_t)port;
    put(&p, 2);
  }
  auto blob = encode_peer_info(pi);
  uint32_t bl = (uint32_t)blob.size();
  put(&bl, 4);
  put(blob.data(), bl);
  return out;
}

bool decode_worker_address(const std::vector<uint8_t>& in,
                                  std::vector<std::pair<std::string, int>>* addrs,
                                  PeerInfo* pi) {
  if (in.size() < 10 || memcmp(in.data(), kAddrMagic, 8) != 0) return false;
  size_t off = 8;
  uint16_t n;
  memcpy(&n, in.data() + off, 2);
  off += 2;
  for (int i = 0; i < n; i++) {
    if (off + 1 > in.size()) return false;
    uint8_t il = in[off++];
    if (off + il + 2 > in.size()) return false;
    std::string ip((const char*)in.data() + off, il);
    off += il;
    uint16_t port;
    memcpy(&port, in.data() + off, 2);
    off += 2;
    addrs->emplace_back(ip, port);
  }
  if (off + 4 > in.size()) return false;
  uint32_t bl;
  memcpy(&bl, in.data() + off, 4);
  off += 4;
  if (off + bl > in.size()) return false;
  return decode_peer_info(in.data() + off, bl, pi);
}

PeerInfo self_peer_info(const std::string& name) {
  PeerInfo pi;
  pi.pid = (uint64_t)getpid();
  memcpy(pi.uuid, process_uuid(), 16);
  memcpy(pi.host_id, host_id(), 16);
  pi.has_gpu = gpu::available();
  pi.gpu_count = gpu::device_count();
  pi.name = name;
  return pi;
}

Connection* Engine::make_listener(const std::string& addr, int port) {
  int fd = ::socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
  if (fd < 0) throw std::runtime_error("socket() failed");
  int one = 1;
  setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
  struct sockaddr_in sin {};
  sin.sin_family = AF_INET;
  sin.sin_port = htons((uint16_t)port);
  if (inet_pton(AF_INET, addr.c_str(), &sin.sin_addr) != 1) {
    ::close(fd);
    throw std::runtime_error("invalid listen address: " + addr);
  }
  if (::bind(fd, (struct sockaddr*)&sin, sizeof(sin)) != 0) {
    ::close(fd);
    throw std::runtime_error("bind failed on " + addr + ":" +
                             std::to_string(port) + ": " + strerror(errno));
  }
  if (::listen(fd, 128) != 0) {
    ::close(fd);
    throw std::runtime_error("listen failed: " + std::string(strerror(errno)));
  }
  struct sockaddr_in got {};
  socklen_t gl = sizeof(got);
  getsockname(fd, (struct sockaddr*)&got, &gl);
  listen_port_ = ntohs(got.sin_port);
  listen_host_ = addr;
  set_nonblocking(fd);
  listen_fd_ = fd;
  return nullptr;
}

void Engine::do_connect_start() {
  // Blocking-ish connect with handshake, abortable via status_==3.
  auto fail = [&](const std::string& why) {
    Completion comp;
    comp.kind = Completion::Kind::Connect;
    comp.error = "not connected: " + why;
    comp.cb0 = py::object();
    {
      py::gil_scoped_acquire gil;
      try {
        if (connect_cb_.ptr()) connect_cb_(comp.error);
      } catch (py::error_already_set& e) {
        e.discard_as_unraisable("starway connect callback");
      }
      connect_cb_ = py::object();
    }
    status_.store(4, std::memory_order_release);
  };

  // Route candidates: worker-address mode may advertise several host IPs;
  // they are tried round-robin until one connects.
  if (connect_candidates_.empty())
    connect_candidates_.emplace_back(connect_host_, connect_port_);
  size_t cand_idx = 0;

  // Connect with a bounded budget (STARWAY_CONNECT_TIMEOUT seconds,
  // default 8); ECONNREFUSED is retried within it (the peer may still be
  // starting up — common in spawn-subprocess tests and rank rendezvous).
  auto deadline = std::chrono::steady_clock::now() +
                  std::chrono::seconds(
                      (long)env_u64("STARWAY_CONNECT_TIMEOUT", 8));
  int fd = -1;
  std::string last_err = "connect TIMEOUT";
  while (fd < 0) {
    if (status_.load(std::memory_order_acquire) == 3) return fail("canceled");
    if (std::chrono::steady_clock::now() > deadline) return fail(last_err);
    auto& [host, port] = connect_candidates_[cand_idx % connect_candidates_.size()];
    cand_idx++;
    connect_host_ = host;
    connect_port_ = port;
    struct sockaddr_in sin {};
    sin.sin_family = AF_INET;
    sin.sin_port = htons((uint16_t)port);
    if (inet_pton(AF_INET, host.c_str(), &sin.sin_addr) != 1) {
      last_err = "invalid address " + host;
      continue;
    }
    int s = ::socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (s < 0) return fail("socket() failed");
    set_nonblocking(s);
    set_tcp_opts(s);
    int r = ::connect(s, (struct sockaddr*)&sin, sizeof(sin));
    int cerr = 0;
    if (r == 0) {
      fd = s;
      break;
    }
    if (errno == EINPROGRESS) {
      while (true) {
        if (status_.load(std::memory_order_acquire) == 3) {
          ::close(s);
          return fail("canceled");
        }
        struct pollfd pfd {s, POLLOUT, 0};
        int pr = ::poll(&pfd, 1, 20);
        if (pr > 0) {
          socklen_t el = sizeof(cerr);
          getsockopt(s, SOL_SOCKET, SO_ERROR, &cerr, &el);
          break;
        }
        if (std::chrono::steady_clock::now() > deadline) {
          ::close(s);
          return fail("connect TIMEOUT");
        }
      }
    } else {
      cerr = errno;
    }
    if (cerr == 0) {
      fd = s;
      break;
    }
    ::close(s);
    last_err = std::string("connect: ") + strerror(cerr);
    if (cerr != ECONNREFUSED && cerr != ENETUNREACH && cerr != EHOSTUNREACH &&
        cerr != ETIMEDOUT)
      return fail(last_err);
    // refused/unreachable: rotate to the next candidate; back off only
    // once all candidates were tried this round.
    if (cand_idx % connect_candidates_.size() == 0) usleep(20000);
  }

  auto c = std::make_unique<Connection>();
  c->fd = fd;
  c->conn_id = next_conn_id_++;
  struct sockaddr_in la {};
  socklen_t ll = sizeof(la);
  getsockname(fd, (struct sockaddr*)&la, &ll);
  char ab[INET_ADDRSTRLEN];
  inet_ntop(AF_INET, &la.sin_addr, ab, sizeof(ab));
  c->local_addr = ab;
  c->local_port = ntohs(la.sin_port);
  c->remote_addr = connect_host_;
  c->remote_port = connect_port_;
  Connection* cp = c.get();
  conns_.push_back(std::move(c));
  send_hello(cp);

  // Drive IO until HELLO exchanged (10 s budget).
  deadline = std::chrono::steady_clock::now() + std::chrono::seconds(10);
  while (!cp->hello_received) {
    if (status_.load(std::memory_order_acquire) == 3 || cp->dead) {
      return fail("canceled or peer reset during handshake");
    }
    bool did = false;
    poll_sockets(5, did);
    if (std::chrono::steady_clock::now() > deadline)
      return fail("handshake TIMEOUT");
  }
  status_.store(2, std::memory_order_release);
  {
    py::gil_scoped_acquire gil;
    try {
      if (connect_cb_.ptr()) connect_cb_(std::string(""));
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("starway connect callback");
    }
    connect_cb_ = py::object();
  }
}

// ---- socket IO ------------------------------------------------------------

void Engine::poll_sockets(int timeout_ms, bool& did_work) {
  std::vector<struct pollfd> pfds;
  pfds.push_back({wake_fds_[0], POLLIN, 0});
  size_t listener_idx = SIZE_MAX;
  if (listen_fd_ >= 0) {
    listener_idx = pfds.size();
    pfds.push_back({listen_fd_, POLLIN, 0});
  }
  size_t conn_base = pfds.size();
  const uint64_t ucap = unexp_cap();
  std::vector<Connection*> live;
  for (auto& c : conns_) {
    if (c->dead || c->fd < 0) continue;
    // Receive window: over the unexpected-staging cap, stop reading this
    // connection (socket backpressure) but keep writing our own frames.
    short ev =
        (ucap && c->unexp_staged_bytes >= ucap) ? 0 : (short)POLLIN;
    if (c->want_write()) ev |= POLLOUT;
    if (!ev) continue;
    pfds.push_back({c->fd, ev, 0});
    live.push_back(c.get());
  }
  int r = ::poll(pfds.data(), (nfds_t)pfds.size(), timeout_ms);
  if (r <= 0) return;
  if (pfds[0].revents & POLLIN) {
    char buf[256];
    while (::read(wake_fds_[0], buf, sizeof(buf)) > 0) {
    }
  }
  if (listener_idx != SIZE_MAX && (pfds[listener_idx].revents & POLLIN))
    accept_new(did_work);
  for (size_t i = 0; i < live.size(); i++) {
    short re = pfds[conn_base + i].revents;
    Connection* c = live[i];
    if (re & (POLLIN | POLLERR | POLLHUP)) handle_readable(c, did_work);
    if (!c->dead && (re & POLLOUT)) handle_writable(c, did_work);
  }
}

void Engine::accept_new(bool& did_work) {
  while (true) {
    struct sockaddr_in ra {};
    socklen_t rl = sizeof(ra);
    int fd = ::accept4(listen_fd_, (struct sockaddr*)&ra, &rl, SOCK_CLOEXEC);
    if (fd < 0) break;
    set_nonblocking(fd);
    set_tcp_opts(fd);
    auto c = std::make_unique<Connection>();
    c->fd = fd;
    c->conn_id = next_conn_id_++;
    char ab[INET_ADDRSTRLEN];
    inet_ntop(AF_INET, &ra.sin_addr, ab, sizeof(ab));
    c->remote_addr = ab;
    c->remote_port = ntohs(ra.sin_port);
    struct sockaddr_in la {};
    socklen_t ll = sizeof(la);
    getsockname(fd, (struct sockaddr*)&la, &ll);
    inet_ntop(AF_INET, &la.sin_addr, ab, sizeof(ab));
    c->local_addr = ab;
    c->local_port = ntohs(la.sin_port);
    conns_.push_back(std::move(c));
    // HELLO handshake is responder-style: the server replies only after
    // registering the endpoint, so by the time the client's connect
    // completes, list_clients() already shows it (reference contract,
    // tests/test_basic.py:43-58).
    did_work = true;
  }
}

void Engine::send_hello(Connection* c) {
  PeerInfo pi = self_peer_info(mode_ == ServerMode ? "server" : "client");
  auto blob = encode_peer_info(pi);
  enqueue_frame(c, FT_HELLO, 0, 0, 0, blob.data(), blob.size(),
                /*priority=*/true);
  c->hello_sent = true;
}

void Engine::handle_readable(Connection* c, bool& did_work) {
  if (c->shm_rx) {
    // Post-switch the socket carries no frames: drain it only to detect
    // peer death (EOF/RST). The peer's closing FIN can arrive BEFORE its
    // remaining ring frames are consumed — defer connection death until
    // the ring drains (the engine-loop EOF check below finishes the job).
    char scratch[4096];
    while (c->fd >= 0) {
      ssize_t n = ::read(c->fd, scratch, sizeof(scratch));
      if (n > 0) continue;
      if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) return;
      // EOF or error: stop polling the socket; ring may still hold data.
      ::close(c->fd);
      c->fd = -1;
      c->sock_eof = true;
      return;
    }
    return;
  }
  handle_stream(c, /*from_ring=*/false, did_work);
}

// Shared frame parser over either byte source. The shm handover switches
// the source exactly at a frame boundary (SHM_ACK / SHM_SWITCH markers),
// so one parser state machine serves both.
void Engine::handle_stream(Connection* c, bool from_ring, bool& did_work) {
  auto src_read = [&](void* dst, size_t want) -> ssize_t {
    if (from_ring) {
      size_t n = c->shm->rx.read(dst, want);
      if (n == 0) return c->shm->rx.peer_closed() ? 0 : -2;
      return (ssize_t)n;
    }
    ssize_t n = ::read(c->fd, dst, want);
    if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) return -2;
    return n;
  };
  const uint64_t ucap = unexp_cap();
  while (!c->dead) {
    // A mid-stream rx-source switch (SHM_SWITCH parsed from TCP) hands the
    // remaining frames to the ring reader invoked from the engine loop.
    if (c->shm_rx != from_ring) return;
    // Receive window: stop consuming at the next frame boundary once the
    // unexpected backlog crosses the cap (bounds overshoot to one message;
    // parser state is preserved and resumes when recvs drain the backlog).
    if (ucap && c->unexp_staged_bytes >= ucap &&
        c->rx_state == Connection::RxState::Header && c->rx_got == 0)
      return;
    if (c->rx_state == Connection::RxState::Header) {
      uint8_t* hp = (uint8_t*)&c->rx_hdr;
      ssize_t n = src_read(hp + c->rx_got, sizeof(FrameHeader) - c->rx_got);
      if (n == -2) return;
      if (n <= 0) {
        on_conn_dead(c);
        return;
      }
      did_work = true;
      c->rx_got += (size_t)n;
      if (c->rx_got < sizeof(FrameHeader)) continue;
      c->rx_got = 0;
      if (c->rx_hdr.magic != kMagic) {
        SW_DBG("bad magic from %s:%d", c->remote_addr.c_str(), c->remote_port);
        on_conn_dead(c);
        return;
      }
      on_frame(c);
    } else {
      // Payload streaming.
      size_t want;
      uint8_t* dst;
      if (c->rx_hdr.type == FT_EAGER) {
        uint64_t done = c->rx_hdr.size - c->rx_msg_remaining;
        if (c->rx_recv_op && !c->rx_truncated) {
          // Zero-copy into the posted buffer (or its host bounce for GPU).
          if (c->rx_recv_op->buf.device >= 0) {
            dst = c->rx_gpu_bounce.data() + done;
          } else {
            dst = c->rx_recv_op->buf.ptr + done;
          }
        } else if (c->rx_unexp && !c->rx_discarding) {
          dst = (c->rx_unexp->redirect_dst ? c->rx_unexp->redirect_dst
                                           : c->rx_unexp->data.data()) +
                done;
        } else {
          if (c->rx_discard.size() < (64 << 10)) c->rx_discard.resize(64 << 10);
          dst = c->rx_discard.data();
        }
        want = c->rx_msg_remaining;
        if ((!c->rx_recv_op || c->rx_truncated) && !c->rx_unexp)
          want = std::min<size_t>(want, c->rx_discard.size());
      } else {
        dst = c->rx_small.data() + c->rx_got;
        want = c->rx_hdr.size - c->rx_got;
      }
      ssize_t n = src_read(dst, want);
      if (n == -2) return;
      if (n <= 0) {
        on_conn_dead(c);
        return;
      }
      did_work = true;
      if (c->rx_hdr.type == FT_EAGER) {
        c->rx_msg_remaining -= (uint64_t)n;
        if (c->rx_unexp) c->rx_unexp->got += (uint64_t)n;
        if (c->rx_msg_remaining == 0) finish_eager_into_recv(c);
      } else {
        c->rx_got += (size_t)n;
        if (c->rx_got == c->rx_hdr.size) {
          c->rx_got = 0;
          c->rx_state = Connection::RxState::Header;
          on_frame_payload(c);
        }
      }
    }
  }
}

void Engine::on_frame(Connection* c) {
  FrameHeader& h = c->rx_hdr;
  switch (h.type) {
    case FT_EAGER:
      begin_eager(c);
      return;
    case FT_SMSG:
      if (h.flags & 1) {
        // Inbox bring-up probe: verify the seq word actually landed in
        // our ring (one unpack of zero bytes), then acknowledge with a
        // CREDIT so the sender activates the plane. Failure = plane
        // stays off for this connection (fail-closed), loudly.
        c->inbox_seen_seq = h.op_id;
        gpu::UnpackMsg um{h.op_id, 0, nullptr};
        std::string err;
        void* t =
            gpu::inbox_unpack(c->inbox_l, &um, 1, engine_lane_, &err);
        if (t) {
          auto batch = std::make_unique<UnpackBatch>();
          batch->ticket = t;
          batch->conn = c;
          batch->msgs.push_back(
              PendingUnpack{c, h.op_id, 0, 0, nullptr, nullptr});
          batch->done.assign(1, false);
          batch->remaining = 1;
          batch->probe = true;
          unpack_batches_.push_back(std::move(batch));
        } else {
          fprintf(stderr, "[starway] inbox probe unpack failed: %s\n",
                  err.c_str());
        }
        return;
      }
      handle_smsg(c, h.tag, h.aux, h.op_id);
      return;
    case FT_INBOX_CREDIT:
      if (h.aux > c->inbox_credit_base) c->inbox_credit_base = h.aux;
      if (!c->inbox_r_active && c->inbox_r.slots &&
          c->inbox_credit_base >= 1) {
        // Bring-up probe acknowledged: the push plane is proven live.
        c->inbox_r_active = true;
        if (c->ep) c->ep->transports.emplace_back("xgmi", "inbox_push");
      }
      return;
    case FT_HELLO:
    case FT_RTS:
    case FT_RTS_INDEXED:
    case FT_RTS_CPU:
    case FT_RECV_FAIL:
    case FT_SHM_OFFER:
    case FT_INBOX_OFFER:
      if (h.size > (16 << 20)) {
        on_conn_dead(c);
        return;
      }
      c->rx_small.resize(h.size);
      c->rx_got = 0;
      c->rx_state = Connection::RxState::Payload;
      if (h.size == 0) {
        c->rx_state = Connection::RxState::Header;
        on_frame_payload(c);
      }
      return;
    case FT_RECV_DONE:
      on_gpu_send_acked(h.op_id, false, "");
      return;
    case FT_FLUSH_REQ:
      // TCP ordering: by the time we parse this, all earlier bytes on this
      // stream have been consumed by the engine => safe to ack.
      enqueue_frame(c, FT_FLUSH_ACK, 0, h.op_id, 0, nullptr, 0, true);
      return;
    case FT_FLUSH_ACK:
      return;  // legacy; flushes complete on write totals
    case FT_SHM_ACK:
      // Client accepted (flags 0) or declined (flags 1) the shm channel.
      // This was the client's LAST tcp frame: subsequent client frames
      // arrive on the ring.
      if (h.flags == 0 && c->shm) {
        enqueue_frame(c, FT_SHM_SWITCH, 0, 0, 0, nullptr, 0, false);
        c->shm_tx_enq = true;  // frames after SWITCH ride the ring
        c->shm_rx = true;
        if (c->ep) c->ep->transports.emplace_back("sm", "shm_ring");
      } else {
        c->shm.reset();
      }
      return;
    case FT_SHM_SWITCH:
      // Server's LAST tcp frame; its later frames arrive on the ring.
      c->shm_rx = true;
      return;
    case FT_BYE:
      on_conn_dead(c);
      return;
    default:
      on_conn_dead(c);
      return;
  }
}

void Engine::on_frame_payload(Connection* c) {
  FrameHeader& h = c->rx_hdr;
  switch (h.type) {
    case FT_HELLO: {
      PeerInfo pi;
      if (!decode_peer_info(c->rx_small.data(), c->rx_small.size(), &pi)) {
        on_conn_dead(c);
        return;
      }
      c->peer = pi;
      c->hello_received = true;
      client_peer_traits_.store(
          (pi.has_gpu ? 1 : 0) |
              (memcmp(pi.uuid, process_uuid(), 16) == 0 ? 2 : 0),
          std::memory_order_release);
      on_hello(c);
      break;
    }
    case FT_RTS: {
      if (c->rx_small.size() != sizeof(RtsDesc)) {
        on_conn_dead(c);
        return;
      }
      RtsDesc rts;
      memcpy(&rts, c->rx_small.data(), sizeof(rts));
      handle_rts(c, rts, IndexRef{}, h.tag, h.aux, h.op_id);
      break;
    }
    case FT_RTS_INDEXED: {
      // The descriptor is for the pool's base; the list travels with it as
      // host bytes, so nothing of the index is read through hipIpc.
      IndexRef src_index;
      std::string err;
      if (!decode_rts_indexed(c->rx_small.data(), c->rx_small.size(),
                              sizeof(RtsDesc), h.aux, &src_index, &err)) {
        SW_DBG("%s", err.c_str());
        on_conn_dead(c);
        return;
      }
      RtsDesc rts;
      memcpy(&rts, c->rx_small.data(), sizeof(rts));
      handle_rts(c, rts, src_index, h.tag, h.aux, h.op_id);
      break;
    }
    case FT_RTS_CPU: {
      if (c->rx_small.size() != sizeof(CmaDesc)) {
        on_conn_dead(c);
        return;
      }
      CmaDesc cma;
      memcpy(&cma, c->rx_small.data(), sizeof(cma));
      // Match like any other message; unmatched waits in the unexpected
      // queue as a descriptor.
      if (Op* r = take_matching_recv(h.tag)) {
        start_cma_pull(r, cma, h.tag, h.aux, h.op_id, c);
      } else {
        UnexpectedMsg* um = park_unexpected(c, h.tag, h.aux, h.op_id);
        um->is_cma = true;
        um->cma = cma;
      }
      break;
    }
    case FT_RECV_FAIL: {
      std::string err((const char*)c->rx_small.data(), c->rx_small.size());
      on_gpu_send_acked(h.op_id, true, err);
      break;
    }
    case FT_INBOX_OFFER: {
      if (c->rx_small.size() != sizeof(gpu::InboxInfo)) break;
      memcpy(&c->inbox_r, c->rx_small.data(), sizeof(gpu::InboxInfo));
      if (c->inbox_r.slots && c->inbox_r.slot_bytes > gpu::kInboxHdrBytes &&
          gpu::available()) {
        // FAIL-CLOSED bring-up: the ring activates only after a seq-1
        // probe round-trips (push over xGMI -> peer unpack -> CREDIT).
        // If the cross-device path misbehaves, the connection simply
        // keeps using the proven RTS rendezvous plane.
        c->inbox_r_active = false;
        c->inbox_next_seq = 2;  // seq 1 is the probe
        c->inbox_credit_base = 0;
        bool same_proc = memcmp(c->peer.uuid, process_uuid(), 16) == 0;
        int run_dev = preferred_device_ >= 0 ? preferred_device_ : 0;
        gpu::PushMsg probe{nullptr, 0, 1, 0};
        std::string err;
        void* ticket = gpu::inbox_push(c->inbox_r, same_proc, run_dev,
                                       &probe, 1, engine_lane_, &err);
        if (ticket) {
          auto batch = std::make_unique<PushBatch>();
          batch->ticket = ticket;
          batch->conn = c;  // no ops: progress_pushes just frees it
          push_batches_.push_back(std::move(batch));
          enqueue_frame(c, FT_SMSG, 0, 1, 0, nullptr, 0, false,
                        /*flags=*/1);
        } else {
          SW_DBG("inbox probe push failed: %s", err.c_str());
        }
      }
      break;
    }
    case FT_SHM_OFFER: {
      // payload: u64 cap | shm name. Client side: map and ACK (accept) or
      // decline; the ACK is this side's last tcp frame on accept.
      bool ok = false;
      if (c->rx_small.size() > 8 && shm_enabled()) {
        uint64_t cap;
        memcpy(&cap, c->rx_small.data(), 8);
        std::string name((const char*)c->rx_small.data() + 8,
                         c->rx_small.size() - 8);
        std::string err;
        ShmChannel* ch = ShmChannel::open(name, cap, &err);
        if (ch) {
          c->shm.reset(ch);
          ok = true;
        } else {
          SW_DBG("shm open failed: %s", err.c_str());
        }
      }
      // Enqueued BEFORE shm_tx_enq flips, so the ACK itself is a tcp frame
      // and everything after it rides the ring. (A write error inside
      // enqueue_frame kills the connection and already reset the flag.)
      enqueue_frame(c, FT_SHM_ACK, 0, 0, 0, nullptr, 0, false,
                    /*flags=*/ok ? 0 : 1);
      if (ok && !c->dead) c->shm_tx_enq = true;
      break;
    }
    default:
      break;
  }
}

void Engine::on_hello(Connection* c) {
  if (mode_ == ServerMode) {
    auto ep = std::make_shared<EndpointInfo>();
    ep->name = "ep-" + std::to_string(c->conn_id) + "@" + c->remote_addr + ":" +
               std::to_string(c->remote_port);
    ep->local_addr = c->local_addr;
    ep->local_port = c->local_port;
    ep->remote_addr = c->remote_addr;
    ep->remote_port = c->remote_port;
    ep->conn = c;
    ep->owner = this;
    ep->peer_has_gpu = c->peer.has_gpu;
    ep->peer_same_proc = memcmp(c->peer.uuid, process_uuid(), 16) == 0;
    ep->transports.emplace_back("tcp", "sock");
    if (gpu::available() && c->peer.has_gpu) {
      bool same_proc = memcmp(c->peer.uuid, process_uuid(), 16) == 0;
      ep->transports.emplace_back("xgmi", same_proc ? "p2p" : "hipipc");
      ep->transports.emplace_back("hbm", "gfx950_copy");
    }
    c->ep = ep;
    {
      std::lock_guard<std::mutex> lk(ep_mu_);
      eps_.push_back(ep);
    }
    send_hello(c);  // responder reply; unblocks the client's connect
    // Same-host peer: offer the shared-memory ring channel (disable with
    // STARWAY_SHM=0 — any value set disables; unset enables).
    if (memcmp(c->peer.host_id, host_id(), 16) == 0 && shm_enabled()) {
      static std::atomic<uint64_t> shm_seq{1};
      uint64_t cap = env_u64("STARWAY_SHM_RING", 8 << 20);
      // round up to a power of two (ring indexing masks with cap-1)
      uint64_t p2 = 4096;
      while (p2 < cap) p2 <<= 1;
      cap = p2;
      char name[96];
      snprintf(name, sizeof(name), "/sw-%d-%llu-%llu", (int)getpid(),
               (unsigned long long)c->conn_id,
               (unsigned long long)shm_seq.fetch_add(1));
      std::string err;
      ShmChannel* ch = ShmChannel::create(name, cap, &err);
      if (ch) {
        c->shm.reset(ch);
        std::vector<uint8_t> payload(8 + strlen(name));
        memcpy(payload.data(), &cap, 8);
        memcpy(payload.data() + 8, name, strlen(name));
        enqueue_frame(c, FT_SHM_OFFER, 0, 0, 0, payload.data(),
                      payload.size(), false);
      } else {
        SW_DBG("shm create failed: %s", err.c_str());
      }
    }
    if (have_accept_cb_) {
      Completion comp;
      comp.kind = Completion::Kind::Accept;
      comp.ep = ep;
      complete(std::move(comp));
    }
  }
  // Small-message inbox: both sides offer their ring to any same-host GPU
  // peer (including same-process loopback, which uses the raw pointer).
  // STARWAY_INBOX=0 disables.
  if (inbox_enabled() && gpu::available() && c->peer.has_gpu &&
      memcmp(c->peer.host_id, host_id(), 16) == 0 && !c->inbox_l_active) {
    std::string err;
    if (gpu::inbox_create(&c->inbox_l, preferred_device_, &err)) {
      c->inbox_l_active = true;
      enqueue_frame(c, FT_INBOX_OFFER, 0, 0, 0, &c->inbox_l,
                    sizeof(gpu::InboxInfo), false);
    } else {
      SW_DBG("inbox create failed: %s", err.c_str());
    }
  }
}

// ---- eager path -----------------------------------------------------------

void Engine::begin_eager(Connection* c) {
  uint64_t msg_len = c->rx_hdr.size;
  uint64_t tag = c->rx_hdr.tag;
  c->rx_recv_op = nullptr;
  c->rx_unexp = nullptr;
  c->rx_truncated = false;
  c->rx_discarding = false;
  c->rx_msg_remaining = msg_len;

  // Match against posted recvs in FIFO order.
  if (Op* r = take_matching_recv(tag)) {
    {
      if (!r->buf.accepts(msg_len) || !r->buf.whole_elems(msg_len)) {
        // Truncation / strided-geometry mismatch / a reducing recv offered
        // part of an element: consume + fail
        // (UCX MESSAGE_TRUNCATED analog; a strided window needs the exact
        // message size or partial rows would smear).
        c->rx_truncated = true;
        c->rx_recv_op = r;
      } else {
        c->rx_recv_op = r;
        if (r->buf.device >= 0 && !c->rx_gpu_bounce.alloc(msg_len)) {
          // Cannot stage the host bounce: fail the recv, then consume and
          // discard the stream bytes (truncation machinery reused with the
          // op already failed).
          c->rx_recv_op = nullptr;
          fail_op(r, "receive failed: host bounce allocation failed");
          c->rx_state =
              msg_len ? Connection::RxState::Payload : Connection::RxState::Header;
          c->rx_discarding = true;
          return;
        }
      }
      c->rx_recv_op->recv_sender_tag = tag;
      c->rx_recv_op->recv_len = msg_len;
    }
  }
  if (!c->rx_recv_op) {
    stats_.unexpected_rx.fetch_add(1, std::memory_order_relaxed);
    auto um = std::make_unique<UnexpectedMsg>();
    um->tag = tag;
    um->size = msg_len;
    um->conn = c;
    if (!um->data.alloc(msg_len)) {
      // Cannot stage it: drop the connection rather than the process.
      SW_DBG("unexpected staging alloc failed (%llu bytes)",
             (unsigned long long)msg_len);
      on_conn_dead(c);
      return;
    }
    // Flow control: staged bytes count against the connection's receive
    // window; past STARWAY_UNEXP_CAP the engine stops reading this
    // connection until recvs drain the backlog (TCP/ring backpressure
    // reaches the sender instead of unbounded staging growth).
    um->staged = msg_len;
    c->unexp_staged_bytes += msg_len;
    stats_.unexp_staged_bytes.fetch_add(msg_len, std::memory_order_relaxed);
    c->rx_unexp = um.get();
    unexpected_.push_back(std::move(um));
  }
  if (msg_len == 0) {
    finish_eager_into_recv(c);
  } else {
    c->rx_state = Connection::RxState::Payload;
  }
}

void Engine::finish_eager_into_recv(Connection* c) {
  c->rx_state = Connection::RxState::Header;
  c->rx_got = 0;
  if (c->rx_discarding) {
    c->rx_discarding = false;
    return;
  }
  if (c->rx_recv_op) {
    Op* r = c->rx_recv_op;
    c->rx_recv_op = nullptr;
    if (c->rx_truncated) {
      c->rx_truncated = false;
      // Same order as every other plane: too long first.
      const bool fits = r->buf.accepts(r->recv_len);
      fail_op(r, "receive failed: " +
                     (fits ? reduce_len_msg(r->recv_len, r->buf)
                           : truncated_msg(r->recv_len, r->buf.capacity())));
      return;
    }
    if (r->buf.device >= 0) {
      upload_to_recv(r, r->recv_sender_tag, r->recv_len,
                     std::move(c->rx_gpu_bounce));
      return;
    }
    deliver_recv(r, r->recv_sender_tag, r->recv_len, RxPlane::Eager);
  } else if (c->rx_unexp) {
    c->rx_unexp->complete = true;
    UnexpectedMsg* um = c->rx_unexp;
    c->rx_unexp = nullptr;
    if (um->bound_recv) {
      Op* r = um->bound_recv;
      um->bound_recv = nullptr;
      // Transfer ownership out of the unexpected queue before delivering.
      for (auto it = unexpected_.begin(); it != unexpected_.end(); ++it) {
        if (it->get() == um) {
          it->release();
          unexpected_.erase(it);
          break;
        }
      }
      complete_recv_from_unexpected(r, um);
    }
  }
}

// ---- tx -------------------------------------------------------------------

void Engine::enqueue_frame(Connection* c, FrameType t, uint64_t tag,
                           uint64_t op_id, uint64_t aux, const void* payload,
                           size_t payload_len, bool priority,
                           uint16_t flags) {
  if (c->dead) return;
  TxItem item;
  item.head.resize(sizeof(FrameHeader) + payload_len);
  FrameHeader h{};
  h.magic = kMagic;
  h.type = t;
  h.flags = flags;
  h.tag = tag;
  h.size = payload_len;
  h.op_id = op_id;
  h.aux = aux;
  memcpy(item.head.data(), &h, sizeof(h));
  if (payload_len) memcpy(item.head.data() + sizeof(h), payload, payload_len);
  item.is_data = (t == FT_RTS || t == FT_RTS_INDEXED);
  item.via_ring = c->shm_tx_enq;
  item.priority = priority;
  c->tx_enqueued_bytes += item.head.size();
  if (priority && !c->txq.empty()) {
    // Insert at a frame boundary: past the partially-written front frame
    // and past every already-queued priority frame, so priority control
    // frames keep their relative order and never jump a queued handshake
    // marker (SHM_ACK/SHM_SWITCH "last TCP frame" invariant).
    size_t pos = c->tx_front_written > 0 ? 1 : 0;
    while (pos < c->txq.size() && c->txq[pos].priority) pos++;
    c->txq.insert(c->txq.begin() + pos, std::move(item));
  } else {
    c->txq.push_back(std::move(item));
  }
  bool dummy = false;
  handle_writable(c, dummy);  // opportunistic immediate write
}

bool Engine::enqueue_eager(Connection* c, Op* op) {
  TxItem item;
  static const size_t kInline = env_u64("STARWAY_EAGER_INLINE", 4096);
  FrameHeader h{};
  h.magic = kMagic;
  h.type = FT_EAGER;
  h.tag = op->tag;
  h.size = op->buf.size;
  h.op_id = op->id;
  h.aux = op->buf.size;
  item.is_data = true;
  item.via_ring = c->shm_tx_enq;
  if (op->capture.size()) {
    // Retransmission of an already-captured payload (CMA fallback): the
    // snapshot becomes the frame body, zero extra copies.
    item.head.resize(sizeof(h));
    memcpy(item.head.data(), &h, sizeof(h));
    item.ext_own = std::move(op->capture);
    item.ext = item.ext_own.data();
    item.ext_len = op->buf.size;
  } else if (op->buf.size <= kInline) {
    item.head.resize(sizeof(h) + op->buf.size);
    memcpy(item.head.data(), &h, sizeof(h));
    memcpy(item.head.data() + sizeof(h), op->buf.ptr, op->buf.size);
  } else {
    item.head.resize(sizeof(h));
    memcpy(item.head.data(), &h, sizeof(h));
    item.ext = op->buf.ptr;
    item.ext_len = op->buf.size;
    item.has_keepalive = true;
    item.keepalive = std::move(op->keepalive);  // moved, no refcount touch
  }
  c->tx_enqueued_bytes += item.head.size() + item.ext_len;
  c->txq.push_back(std::move(item));
  bool dummy = false;
  handle_writable(c, dummy);
  // Capture-on-completion: if the zero-copy frame was not fully written by
  // the opportunistic write above, snapshot the unwritten remainder into
  // engine-owned memory before the send completes, so no live pointer into
  // the caller's buffer survives completion (buffer-reuse contract).
  if (!c->txq.empty()) {
    TxItem& back = c->txq.back();
    if (back.ext && back.ext_own.empty() && back.ext == op->buf.ptr) {
      size_t off = 0;
      if (&back == &c->txq.front() && c->tx_front_written > back.head.size())
        off = c->tx_front_written - back.head.size();
      // Capture ceiling (STARWAY_CAPTURE_MAX, default 1 GiB): above it a
      // snapshot would double resident memory, so completion defers to
      // write-out instead (still reuse-safe — the buffer is pinned and
      // the caller's await resolves only once the bytes left).
      static const uint64_t kCaptureMax =
          env_u64("STARWAY_CAPTURE_MAX", 1ull << 30);
      if (back.ext_len - off > kCaptureMax) {
        back.owner = op;
        return false;
      }
      if (back.ext_own.alloc(back.ext_len)) {
        memcpy(back.ext_own.data() + off, back.ext + off, back.ext_len - off);
        back.ext = back.ext_own.data();
        if (back.has_keepalive) {
          dead_objs_.push_back(std::move(back.keepalive));
          back.has_keepalive = false;
        }
      } else {
        // Snapshot allocation failed (enormous payload under memory
        // pressure): keep zero-copy and defer completion to write-out.
        back.owner = op;
        return false;
      }
    }
  }
  return true;
}

void Engine::handle_writable(Connection* c, bool& did_work) {
  while (!c->txq.empty() && !c->dead) {
    TxItem& it = c->txq.front();
    size_t head_off = std::min(c->tx_front_written, it.head.size());
    size_t ext_off = c->tx_front_written - head_off;
    struct iovec iov[2];
    int nio = 0;
    if (head_off < it.head.size()) {
      iov[nio].iov_base = it.head.data() + head_off;
      iov[nio].iov_len = it.head.size() - head_off;
      nio++;
    }
    if (it.ext && ext_off < it.ext_len) {
      iov[nio].iov_base = (void*)(it.ext + ext_off);
      iov[nio].iov_len = it.ext_len - ext_off;
      nio++;
    }
    if (nio == 0) {
      // fully written
    } else if (it.via_ring) {
      size_t wrote = 0;
      for (int k = 0; k < nio; k++) {
        size_t n = c->shm->tx.write(iov[k].iov_base, iov[k].iov_len);
        wrote += n;
        if (n < iov[k].iov_len) break;  // ring full
      }
      if (wrote == 0) return;  // consumer will drain; retried by the loop
      did_work = true;
      c->tx_front_written += wrote;
      c->tx_written_bytes += (uint64_t)wrote;
    } else {
      ssize_t n = ::writev(c->fd, iov, nio);
      if (n < 0) {
        if (errno == EAGAIN || errno == EWOULDBLOCK) return;
        on_conn_dead(c);
        return;
      }
      did_work = true;
      c->tx_front_written += (size_t)n;
      c->tx_written_bytes += (uint64_t)n;
    }
    if (c->tx_front_written >= it.head.size() + it.ext_len) {
      if (it.has_keepalive) {
        dead_objs_.push_back(std::move(it.keepalive));
        it.has_keepalive = false;
      }
      if (it.owner) {
        // Deferred-completion eager send: payload now fully on the wire.
        complete_send(it.owner);
        it.owner = nullptr;
      }
      c->txq.pop_front();
      c->tx_front_written = 0;
    } else {
      return;  // kernel buffer full
    }
  }
}

}  // namespace sw
