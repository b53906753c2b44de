// starway_amd GPU layer — hipIpc zero-copy mapping, per-device pull streams,
// hipEvent completion tickets. Replaces what UCX's cuda_copy/rocm transports
// would have done for the reference ("CUDA buffers are planned",
// reference benchmark.md:147) with a native xGMI design:
//   * sender exports (ipc handle, offset) for its device buffer
//   * receiver maps it once (cached) and PULLS with a gfx950 copy kernel
//     running on its own device — a peer read rides xGMI links directly
//   * completion = hipEvent recorded on the pull stream, polled by the
//     engine's progress loop (the ucp_worker_progress analog)
#include "core.hpp"
#include "gpu_hooks.hpp"
#include "gpu_internal.hpp"
#include "kernels.hpp"

#include <dlfcn.h>
#include <sys/stat.h>
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cstring>
#include <tuple>

namespace sw {
namespace gpu {

static std::mutex g_mu;

static int cached_device_count() {
  static int count = [] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return 0;
    return n;
  }();
  return count;
}

bool available() { return cached_device_count() > 0; }

// Current device of the CALLING thread (Python thread at object
// construction), used to place engine-owned device state.
int current_device() {
  if (!available()) return -1;
  int d = 0;
  return hipGetDevice(&d) == hipSuccess ? d : -1;
}
int device_count() { return cached_device_count(); }

// Optional roctx range markers (STARWAY_ROCTX=1): rocprofv3 --marker-trace
// shows named spans around the data-plane operations. Loaded lazily via
// dlopen so the core has no link-time roctracer dependency.
namespace {
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)();
struct Roctx {
  roctx_push_fn push = nullptr;
  roctx_pop_fn pop = nullptr;
  Roctx() {
    const char* v = getenv("STARWAY_ROCTX");
    if (!v || !strcmp(v, "0")) return;
    void* h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
    pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
  }
};
Roctx& roctx() {
  static Roctx r;
  return r;
}
struct RoctxSpan {
  bool active;
  explicit RoctxSpan(const char* name) : active(roctx().push != nullptr) {
    if (active) roctx().push(name);
  }
  ~RoctxSpan() {
    if (active) roctx().pop();
  }
};
}  // namespace

// ---------------------------------------------------------------------------
// Calibrated performance constants (SURVEY §2 replacement-table last row:
// "analytic model + cached microbenchmark calibration"). First use on a
// GPU box runs a ~100 ms copy microbenchmark and persists the result under
// ~/.cache/starway/perf.cal; later processes just read the file. The
// analytic fallbacks are round-1 MI355X measurements.
// ---------------------------------------------------------------------------

struct Calib {
  double same_gbps = 0;
  double xgmi_gbps = 0;
  bool tried = false;
};
static Calib g_calib;  // g_mu NOT required: written once under g_calib_mu
// Bumped whenever the kernel that calibrate() times changes (2: same-device
// copies of 64 MiB and more take the streaming kernel); a perf.cal without
// this version is not trusted.
constexpr int kCalibVersion = 2;
static std::mutex g_calib_mu;

static std::string calib_path() {
  if (const char* p = getenv("STARWAY_CALIB_FILE")) return p;
  const char* h = getenv("HOME");
  return std::string(h ? h : "/tmp") + "/.cache/starway/perf.cal";
}

static void load_calib_locked() {
  FILE* f = fopen(calib_path().c_str(), "r");
  if (!f) return;
  char key[64];
  double val;
  double same = 0, xgmi = 0;
  int version = 0;
  while (fscanf(f, "%63s %lf", key, &val) == 2) {
    if (!strcmp(key, "version")) version = (int)val;
    if (!strcmp(key, "same_gpu_gbps") && val > 0) same = val;
    if (!strcmp(key, "xgmi_gbps") && val > 0) xgmi = val;
  }
  fclose(f);
  // A file written for another production kernel is stale: ignore it, so
  // the next calibration overwrites it.
  if (version != kCalibVersion) return;
  if (same > 0) g_calib.same_gbps = same;
  if (xgmi > 0) g_calib.xgmi_gbps = xgmi;
}

static void free_on(int device, void* p) {
  DeviceGuard on(device);
  hipFree(p);
}

// Timed device copy through the production kernel: dst/src on (possibly
// different) devices, kernel runs on dst_dev (the pull pattern).
static double timed_copy_gbps(int dst_dev, int src_dev, size_t nbytes) {
  void* src = nullptr;
  void* dst = nullptr;
  {
    DeviceGuard on(src_dev);
    if (hipMalloc(&src, nbytes) != hipSuccess) return 0;
    hipMemset(src, 1, nbytes);
  }
  DeviceGuard on(dst_dev);
  if (hipMalloc(&dst, nbytes) != hipSuccess) {
    free_on(src_dev, src);
    return 0;
  }
  if (dst_dev != src_dev) {
    hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
    (void)e;
  }
  hipStream_t s;
  hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  double best = 0;
  for (int rep = 0; rep < 4; rep++) {
    auto t0 = std::chrono::steady_clock::now();
    launch_copy(dst, src, nbytes, s, dst_dev == src_dev);
    hipStreamSynchronize(s);
    double dt = std::chrono::duration<double>(
                    std::chrono::steady_clock::now() - t0)
                    .count();
    double g = (double)nbytes / dt / 1e9;
    if (rep > 0 && g > best) best = g;  // rep 0 = warmup
  }
  hipStreamDestroy(s);
  hipFree(dst);
  free_on(src_dev, src);
  return best;
}

bool calibrate(bool force, std::string* err) {
  std::lock_guard<std::mutex> lk(g_calib_mu);
  if (!available()) {
    if (err) *err = "no HIP device";
    return false;
  }
  if (!force) {
    load_calib_locked();
    if (g_calib.same_gbps > 0) return true;
  }
  const size_t n = 64 << 20;
  double same = timed_copy_gbps(0, 0, n);
  double xgmi = 0;
  if (cached_device_count() >= 2) xgmi = timed_copy_gbps(1, 0, n);
  if (same <= 0) {
    if (err) *err = "calibration copy failed";
    return false;
  }
  g_calib.same_gbps = same;
  if (xgmi > 0) g_calib.xgmi_gbps = xgmi;
  std::string path = calib_path();
  // mkdir -p equivalent (no shell: the path comes from environment vars).
  for (size_t pos = 1; (pos = path.find('/', pos)) != std::string::npos;
       pos++) {
    std::string dir = path.substr(0, pos);
    if (!dir.empty()) mkdir(dir.c_str(), 0755);
  }
  if (FILE* f = fopen(path.c_str(), "w")) {
    fprintf(f, "version %d\n", kCalibVersion);
    fprintf(f, "same_gpu_gbps %.1f\n", g_calib.same_gbps);
    if (g_calib.xgmi_gbps > 0)
      fprintf(f, "xgmi_gbps %.1f\n", g_calib.xgmi_gbps);
    fclose(f);
  }
  return true;
}

static void maybe_calibrate() {
  // Lazy: first perf query on a GPU box loads the cache, running the
  // microbenchmark once if no cache exists (STARWAY_CALIBRATE=0 skips).
  {
    std::lock_guard<std::mutex> lk(g_calib_mu);
    if (g_calib.tried) return;
    g_calib.tried = true;
    if (!available()) return;
    load_calib_locked();
    if (g_calib.same_gbps > 0) return;
    const char* v = getenv("STARWAY_CALIBRATE");
    if (v && !strcmp(v, "0")) return;
  }
  std::string err;
  calibrate(false, &err);
}

double same_gpu_copy_gbps() {
  maybe_calibrate();
  return g_calib.same_gbps > 0 ? g_calib.same_gbps : 3100.0;
}
double xgmi_link_gbps() {
  maybe_calibrate();
  return g_calib.xgmi_gbps > 0 ? g_calib.xgmi_gbps : 140.0;
}

// Device ordinal owning `ptr`, or -1 if not device memory / no GPU.
int device_of(const void* ptr) {
  if (!available()) return -1;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) return -1;
  if (attr.type == hipMemoryTypeDevice) return attr.device;
  return -1;
}

// ---------------------------------------------------------------------------
// per-device streams
// ---------------------------------------------------------------------------

// Pulls from DIFFERENT source peers must overlap (each rides its own xGMI
// link), so streams are keyed by (device, lane) with lane derived from the
// message source; pulls from the same peer share a lane (one link's worth
// of bandwidth anyway, and it keeps per-pair completion work ordered).
// STARWAY_LANES (default 8, power of two): more lanes overlap pulls from
// more peers; fewer lanes reduce the per-device HSA queue count (queue
// oversubscription across many processes sharing one GPU time-slices HW
// queues at ~ms granularity).
static int stream_lanes() {
  static int lanes = [] {
    int v = (int)env_u64("STARWAY_LANES", 8);
    int p2 = 1;
    while (p2 < v && p2 < 16) p2 <<= 1;
    return p2;
  }();
  return lanes;
}

static hipStream_t pull_stream(int device, int lane = 0) {
  static std::map<std::pair<int, int>, hipStream_t> streams;  // g_mu held
  lane &= (stream_lanes() - 1);
  auto key = std::make_pair(device, lane);
  auto it = streams.find(key);
  if (it != streams.end()) return it->second;
  DeviceGuard on(device);
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
    s = nullptr;
  streams[key] = s;
  return s;
}

// ---------------------------------------------------------------------------
// peer access (same-process cross-device pointers)
// ---------------------------------------------------------------------------

static void ensure_peer_access(int dst_dev, int src_dev) {
  if (dst_dev == src_dev) return;
  static std::set<std::pair<int, int>> enabled;  // guarded by g_mu
  auto key = std::make_pair(dst_dev, src_dev);
  if (enabled.count(key)) return;
  DeviceGuard on(dst_dev);
  hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
  (void)e;  // hipErrorPeerAccessAlreadyEnabled is fine
  enabled.insert(key);
}

// ---------------------------------------------------------------------------
// IPC handle caches
// ---------------------------------------------------------------------------

// Export cache: base ptr -> (handle, allocation size). Registration-cache
// pattern: torch's caching allocator keeps blocks alive, so base pointers
// stay valid across messages. Entries are VALIDATED on lookup by comparing
// the allocation size hipMemGetAddressRange reports — a freed-and-reused
// base with a different size re-exports. A reuse at the same base AND the
// same size cannot be detected this way; callers using allocators that
// return memory to the driver mid-run (e.g. torch empty_cache) must call
// starway_amd.ipc_invalidate() (-> ipc_close_all) at that point.
struct ExportEntry {
  hipIpcMemHandle_t handle;
  size_t size = 0;
};
static std::map<void*, ExportEntry> g_export_cache;

// Import cache: (device, 64B handle) -> mapped base. Guarded by its own
// mutex because it is shared between the pull path (g_mu domain) and the
// small-message inbox path (sm_mu domain in smallmsg.hip).
using HandleKey = std::array<uint8_t, kIpcHandleBytes>;
static std::mutex g_ipc_mu;
static std::map<std::pair<int, HandleKey>, void*> g_import_cache;

static void release_index_pool();  // g_mu held

void ipc_close_all() {
  std::lock_guard<std::mutex> lk0(g_mu);
  std::lock_guard<std::mutex> lk(g_ipc_mu);
  for (auto& [key, base] : g_import_cache) {
    DeviceGuard on(key.first);
    hipIpcCloseMemHandle(base);
  }
  g_import_cache.clear();
  g_export_cache.clear();
  // The pooled device index buffers go with the other cached device state
  // (this runs at interpreter exit too).
  release_index_pool();
}

bool make_rts(const BufferRef& buf, RtsDesc* out, std::string* err) {
  RoctxSpan span("starway::make_rts");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available in sender process";
    return false;
  }
  memset(out, 0, sizeof(*out));
  memcpy(out->src_uuid, process_uuid(), 16);
  out->device = buf.device;
  out->raw_ptr = (uint64_t)(uintptr_t)buf.ptr;
  out->src_rows = buf.rows;
  out->src_row_bytes = buf.row_bytes;
  out->src_stride = buf.stride;
  out->src_nd = buf.nd;
  // Resolve the allocation base for IPC export.
  DeviceGuard on(buf.device);
  hipDeviceptr_t base = 0;
  size_t bsize = 0;
  hipError_t e = hipMemGetAddressRange(&base, &bsize, (hipDeviceptr_t)buf.ptr);
  if (e == hipSuccess) {
    auto it = g_export_cache.find((void*)base);
    if (it != g_export_cache.end() && it->second.size != bsize) {
      // Base address reused by a different allocation: stale entry.
      g_export_cache.erase(it);
      it = g_export_cache.end();
    }
    if (it == g_export_cache.end()) {
      ExportEntry ent;
      ent.size = bsize;
      e = hipIpcGetMemHandle(&ent.handle, (void*)base);
      if (e == hipSuccess) {
        it = g_export_cache.emplace((void*)base, ent).first;
      } else {
        it = g_export_cache.end();
      }
    }
    if (it != g_export_cache.end()) {
      out->use_ipc = 1;
      memcpy(out->ipc_handle, &it->second.handle, kIpcHandleBytes);
      out->offset = (uint64_t)((uintptr_t)buf.ptr - (uintptr_t)base);
    }
  }
  // use_ipc==0 is still fine for same-process delivery (raw_ptr path);
  // a cross-process receiver will report the error.
  return true;
}

// ---------------------------------------------------------------------------
// tickets
// ---------------------------------------------------------------------------

// The index lists of one indexed launch on the device: one pooled buffer
// holding the destination's list, then the source's, filled by
// hipMemcpyAsync on the route's stream ahead of the kernel. The ticket owns
// it as it owns staging, and keeps the host lists alive until its event has
// passed (the async copies read them).
struct IndexUpload {
  void* dev = nullptr;
  size_t cap = 0;
  int device = -1;
  std::shared_ptr<const IndexList> host[2];
};

struct Ticket {
  hipEvent_t ev = nullptr;
  int device = -1;
  RawBuf bounce;  // host staging kept alive until completion
  // Contiguous device staging of an N-D or indexed transfer; released with
  // the ticket.
  void* dev_staging = nullptr;
  IndexUpload index;
};

// Device index buffers are pooled per device (g_mu held): a list is at most
// 256 KiB, a message brings at most two, and hipMalloc plus a hipFree that
// may wait for the device would cost more than a small indexed copy.
static std::map<int, std::vector<std::pair<void*, size_t>>> g_index_pool;

// A buffer in use is owned by its ticket, not by the pool.
static void release_index_pool() {
  for (auto& [device, pool] : g_index_pool) {
    DeviceGuard on(device);
    for (auto& buf : pool) hipFree(buf.first);
  }
  g_index_pool.clear();
}

static hipError_t index_buf_get(int device, size_t need, IndexUpload* up) {
  auto& pool = g_index_pool[device];
  for (size_t i = 0; i < pool.size(); i++) {
    if (pool[i].second >= need) {
      up->dev = pool[i].first;
      up->cap = pool[i].second;
      up->device = device;
      pool.erase(pool.begin() + i);
      return hipSuccess;
    }
  }
  size_t cap = 4096;
  while (cap < need) cap <<= 1;
  hipError_t e = hipMalloc(&up->dev, cap);
  if (e != hipSuccess) {
    up->dev = nullptr;
    return e;
  }
  up->cap = cap;
  up->device = device;
  return hipSuccess;
}

// Release staging and index buffer of a route that ends without a ticket;
// work queued on `stream` may still touch either.
static void abandon_route(void* staging, IndexUpload* up, hipStream_t stream);

// Hand the buffer back once nothing on the device can still read it:
// `idle` false means a kernel or copy using it may be in flight, and the
// buffer is freed (hipFree waits) instead of pooled.
static void index_buf_put(IndexUpload* up, bool idle) {
  if (up->dev) {
    auto& pool = g_index_pool[up->device];
    if (idle && pool.size() < 16)
      pool.emplace_back(up->dev, up->cap);
    else
      hipFree(up->dev);
  }
  *up = IndexUpload{};
}

// hipMemcpy2DAsync cannot express an N-D layout, so a host endpoint of an
// N-D device buffer goes through a contiguous device staging buffer on the
// same stream: host -> staging -> k_copy_nd -> destination, or the
// reverse. Not the hot path (device<->device pulls never stage): a plain
// hipMalloc per transfer, and a hipFree that may wait for the device.
static hipError_t alloc_staging(uint64_t size, void** out) {
  return hipMalloc(out, size ? size : 1);
}

// Release a staging buffer whose ticket was never handed out; work queued
// on `stream` may still touch it.
static void drop_staging(void* staging, hipStream_t stream) {
  if (!staging) return;
  hipStreamSynchronize(stream);
  hipFree(staging);
}

static void abandon_route(void* staging, IndexUpload* up,
                          hipStream_t stream) {
  drop_staging(staging, stream);
  if (up && up->dev)
    index_buf_put(up, hipStreamSynchronize(stream) == hipSuccess);
}

// hipEvent pool per device (create/destroy costs ~1-2 us per op).
static std::map<int, std::vector<hipEvent_t>> g_event_pool;

static hipError_t pool_get_event(int device, hipEvent_t* ev) {
  auto& pool = g_event_pool[device];
  if (!pool.empty()) {
    *ev = pool.back();
    pool.pop_back();
    return hipSuccess;
  }
  return hipEventCreateWithFlags(ev, hipEventDisableTiming);
}

static void pool_put_event(int device, hipEvent_t ev) {
  auto& pool = g_event_pool[device];
  if (pool.size() < 256) {
    pool.push_back(ev);
  } else {
    hipEventDestroy(ev);
  }
}

// Map a peer's exported allocation on open_device (cached per device ×
// handle). Shared by the pull path and the small-message inbox push path.
void* import_ipc(const uint8_t* handle, int open_device, std::string* err) {
  std::lock_guard<std::mutex> lk(g_ipc_mu);
  HandleKey key;
  memcpy(key.data(), handle, kIpcHandleBytes);
  auto ck = std::make_pair(open_device, key);
  auto it = g_import_cache.find(ck);
  if (it != g_import_cache.end()) return it->second;
  hipIpcMemHandle_t h;
  memcpy(&h, handle, kIpcHandleBytes);
  void* base = nullptr;
  hipError_t e;
  {
    DeviceGuard on(open_device);
    e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
  }
  if (e != hipSuccess) {
    *err = hip_error("hipIpcOpenMemHandle", e);
    return nullptr;
  }
  g_import_cache[ck] = base;
  return base;
}

// The common tail of every begin_*: the work is queued on `stream`; hand out
// a ticket whose event follows it and that owns `staging`. A failed launch
// (`launched`) or a failed event releases the staging and returns null.
static Ticket* finish_ticket(int device, hipStream_t stream, void* staging,
                             IndexUpload* index, hipError_t launched,
                             const char* launch_what, const char* event_what,
                             std::string* err) {
  if (launched != hipSuccess) {
    abandon_route(staging, index, stream);
    *err = hip_error(launch_what, launched);
    return nullptr;
  }
  Ticket* t = new Ticket();
  t->device = device;
  hipError_t e = pool_get_event(device, &t->ev);
  if (e == hipSuccess) e = hipEventRecord(t->ev, stream);
  if (e != hipSuccess) {
    abandon_route(staging, index, stream);
    delete t;
    *err = hip_error(event_what, e);
    return nullptr;
  }
  t->dev_staging = staging;
  if (index) {
    t->index = *index;
    *index = IndexUpload{};
  }
  return t;
}

// A reducing or converting destination takes whole elements, read in the
// message's element size, into a dense buffer aligned to its own.
static bool check_reduce_dst(const BufferRef& dst, uint64_t size,
                             std::string* err) {
  const size_t es = elem_size(dst.elem);
  const size_t ms = elem_size(dst.msg_type());
  if (dst.dense() && es != 0 && ms != 0 && (uintptr_t)dst.ptr % es == 0 &&
      size % ms == 0 && size / ms <= dst.size / es)
    return true;
  *err = std::string(dst.converting() ? "msg_dtype" : "reduce") +
         ": destination or message length does not fit the element type";
  return false;
}

// A strided window (rows or N-D) or an indexed destination takes exactly
// its own size: a shorter message would smear partial rows or slices.
static bool check_window(const BufferRef& dst, uint64_t size,
                         std::string* err) {
  if (dst.dense() || dst.size == size) return true;
  *err = "strided recv buffer geometry mismatch (buffer " +
         std::to_string(dst.size) + " B, message " + std::to_string(size) +
         " B)";
  return false;
}

// The source of a pull, decoded once from the peer's descriptor: where it
// lies in this process (raw pointer or hipIpc mapping on open_device) and
// its geometry, as a BufferRef of `size` message bytes on rts.device. The
// descriptor comes from the peer, so the geometry is checked here, for
// every route: it must describe exactly `size` bytes.
struct PullSrc {
  BufferRef buf;
  bool same_proc = false;
};

static bool decode_rts(const RtsDesc& rts, const IndexRef& src_index,
                       uint64_t size, int open_device, PullSrc* out,
                       std::string* err) {
  out->same_proc = memcmp(rts.src_uuid, process_uuid(), 16) == 0;
  BufferRef& s = out->buf;
  if (out->same_proc) {
    s.ptr = (uint8_t*)(uintptr_t)rts.raw_ptr;
  } else if (!rts.use_ipc) {
    *err = "peer did not export an IPC handle (cross-process GPU transfer)";
    return false;
  } else {
    void* base = import_ipc(rts.ipc_handle, open_device, err);
    if (!base) return false;
    s.ptr = (uint8_t*)base + rts.offset;
  }
  s.size = size;
  s.device = rts.device;
  if (src_index.on()) {
    // The descriptor is for the pool's base; the list came with it in the
    // frame. The frame decoder has checked it; the sum is checked again
    // here because every route relies on it.
    if (src_index.count() * src_index.slice_bytes != size ||
        src_index.count() > kIndexMax || rts.src_rows > 0 ||
        rts.src_nd.ndim > 0) {
      *err = "malformed indexed source in RTS";
      return false;
    }
    s.index = src_index;
  } else if (rts.src_nd.ndim > 0) {
    s.nd = rts.src_nd;
    if (s.nd.ndim > kMaxDims || s.nd.unit == 0 || layout_bytes(s.nd) != size) {
      *err = "malformed N-D source layout in RTS";
      return false;
    }
  } else if (rts.src_rows > 0) {
    if (rts.src_rows * rts.src_row_bytes != size) {
      *err = "malformed strided source layout in RTS";
      return false;
    }
    s.rows = rts.src_rows;
    s.row_bytes = rts.src_row_bytes;
    s.stride = rts.src_stride;
  }
  return true;
}

// First-contact route self-check: one stderr line per (dst device, src
// device, process locality) triple, so a multi-GPU driver-run failure is
// diagnosable from the log tail (which xGMI pair, ipc vs raw pointer,
// which lane, which copy engine). STARWAY_LOG_ROUTE=0 silences it.
static void log_route_once(int run_dev, const RtsDesc& rts, bool same_proc,
                           int lane, const char* engine) {
  static const bool enabled = [] {
    const char* v = getenv("STARWAY_LOG_ROUTE");
    return !(v && !strcmp(v, "0"));
  }();
  if (!enabled) return;
  // g_mu held by callers. The engine is part of the key: a copy route
  // and an accumulate route over one device pair each get their line.
  static std::set<std::tuple<int, int, int, std::string>> seen;
  if (!seen.insert({run_dev, rts.device, (int)same_proc, engine}).second)
    return;
  fprintf(stderr,
          "[starway] route: pull dev%d <- peer dev%d (%s, %s) lane=%d "
          "engine=%s\n",
          run_dev, rts.device, same_proc ? "same-proc" : "cross-proc",
          rts.use_ipc ? "hipipc" : "raw-ptr", lane, engine);
}

// One launch of the indexed kernel for `size` message bytes on `stream`,
// its lists uploaded ahead of it into `up`. A side whose index is off is
// one dense run; an indexed side's slices must add up to `size`.
static hipError_t copy_indexed(void* dst, const IndexRef& di, const void* src,
                               const IndexRef& si, uint64_t size, int run_dev,
                               hipStream_t stream, const CopyTuning& tuning,
                               IndexUpload* up,
                               IndexWidth width = IndexWidth::Auto) {
  if ((di.on() && di.count() * di.slice_bytes != size) ||
      (si.on() && si.count() * si.slice_bytes != size) || up->dev)
    return hipErrorInvalidValue;
  if (size == 0) return hipSuccess;
  const size_t nd = (size_t)di.count() * sizeof(uint32_t);
  const size_t ns = (size_t)si.count() * sizeof(uint32_t);
  hipError_t e = index_buf_get(run_dev, nd + ns, up);
  if (e != hipSuccess) return e;
  uint8_t* base = (uint8_t*)up->dev;
  IndexSide d{nullptr, 0, 0}, s{nullptr, 0, 0};
  if (di.on()) {
    up->host[0] = di.list;
    e = hipMemcpyAsync(base, di.list->data(), nd, hipMemcpyHostToDevice,
                       stream);
    if (e != hipSuccess) return e;
    d = IndexSide{(const uint32_t*)base, di.slice_bytes, di.stride};
  }
  if (si.on()) {
    up->host[1] = si.list;
    e = hipMemcpyAsync(base + nd, si.list->data(), ns, hipMemcpyHostToDevice,
                       stream);
    if (e != hipSuccess) return e;
    s = IndexSide{(const uint32_t*)(base + nd), si.slice_bytes, si.stride};
  }
  return launch_copy_indexed(dst, d, src, s, size, stream, tuning, width);
}

// Pack a device source of any geometry into fresh contiguous device staging
// with the copy kernel that serves that geometry, on `stream`. `up` takes
// the list of an indexed source.
static hipError_t pack_to_staging(const BufferRef& src, int run_dev,
                                  hipStream_t stream, void** staging,
                                  IndexUpload* up) {
  hipError_t e = alloc_staging(src.size, staging);
  if (e != hipSuccess) return e;
  if (src.index.on())
    return copy_indexed(*staging, IndexRef{}, src.ptr, src.index, src.size,
                        run_dev, stream, default_copy_tuning(), up);
  if (src.nd.ndim > 0)
    return launch_copy_nd(*staging, contiguous_layout(src.size), src.ptr,
                          src.nd, src.size, stream);
  if (src.rows > 0)
    return launch_copy_strided(*staging, src.row_bytes, src.ptr, src.stride,
                               src.rows, src.row_bytes, stream);
  return launch_copy(*staging, src.ptr, src.size, stream,
                     src.device == run_dev);
}

// Fresh device staging filled from `size` host bytes, on `stream`.
static hipError_t stage_from_host(const void* host_src, uint64_t size,
                                  hipStream_t stream, void** staging) {
  hipError_t e = alloc_staging(size, staging);
  if (e == hipSuccess)
    e = hipMemcpyAsync(*staging, host_src, size, hipMemcpyHostToDevice,
                       stream);
  return e;
}

// Device source -> host memory: a contiguous or rows source is read where
// it lies, an N-D or indexed one is packed into device staging first.
static hipError_t download(void* host_dst, const BufferRef& src, int run_dev,
                           hipStream_t stream, void** staging,
                           IndexUpload* up) {
  if (src.nd.ndim > 0 || src.index.on()) {
    hipError_t e = pack_to_staging(src, run_dev, stream, staging, up);
    if (e == hipSuccess)
      e = hipMemcpyAsync(host_dst, *staging, src.size, hipMemcpyDeviceToHost,
                         stream);
    return e;
  }
  if (src.rows > 0)
    return hipMemcpy2DAsync(host_dst, src.row_bytes, src.ptr, src.stride,
                            src.row_bytes, src.rows, hipMemcpyDeviceToHost,
                            stream);
  return hipMemcpyAsync(host_dst, src.ptr, src.size, hipMemcpyDeviceToHost,
                        stream);
}

// `size` message bytes at `from`, aligned to the message's element size,
// into a reducing or converting dst: the accumulate kernels for a message
// of the buffer's own type, the convert kernels for another.
static hipError_t launch_typed(const BufferRef& dst, const void* from,
                               uint64_t size, hipStream_t stream) {
  if (dst.converting())
    return launch_convert(dst.ptr, dst.elem, from, dst.msg_elem,
                          size / elem_size(dst.msg_elem), dst.reducing(),
                          stream);
  return launch_accum(dst.ptr, from, size, dst.elem, stream);
}

// dst += source (reducing), dst = convert(source) (converting) or both, on
// `stream`. The kernel reads an element-aligned contiguous source where it
// lies (peer memory over xGMI, hipIpc-mapped, or local); a rows, N-D,
// indexed or element-misaligned source is packed into staging first (same
// stream, so in order).
static hipError_t accumulate(const BufferRef& dst, const BufferRef& src,
                             int run_dev, hipStream_t stream, void** staging,
                             IndexUpload* up) {
  const void* from = src.ptr;
  if (!src.dense() || (uintptr_t)src.ptr % elem_size(dst.msg_type()) != 0) {
    hipError_t e = pack_to_staging(src, run_dev, stream, staging, up);
    if (e != hipSuccess) return e;
    from = *staging;
  }
  return launch_typed(dst, from, src.size, stream);
}

// One side of an N-D copy of `size` message bytes, as a Layout.
static Layout layout_of(const BufferRef& buf, uint64_t size) {
  return buf.dense() ? contiguous_layout(size) : buf.layout();
}

// The device-to-device copy for a (source, destination) geometry pair, run
// on the destination's device; dst overwritten. False with *err set when
// the pair is refused; else *launched is the launch's status.
//   either side indexed    launch_copy_indexed when the other side is dense
//                          or indexed too; a rows or N-D side opposite an
//                          indexed one goes through contiguous staging: the
//                          source is packed into it by its own kernel, then
//                          the destination's kernel reads from it
//   either side N-D        launch_copy_nd, the other side as a layout
//   else either side rows  launch_copy_strided; two rows sides must agree
//   else (flat)            launch_copy, or SDMA under STARWAY_PULL=sdma
static bool copy_d2d(const BufferRef& dst, const PullSrc& from, uint64_t size,
                     hipStream_t stream, void** staging, IndexUpload* up,
                     hipError_t* launched, std::string* err) {
  const BufferRef& src = from.buf;
  if (src.index.on() || dst.index.on()) {
    const bool src_fits = src.dense() || src.index.on();
    const bool dst_fits = dst.dense() || dst.index.on();
    if (src_fits && dst_fits) {
      *launched = copy_indexed(dst.ptr, dst.index, src.ptr, src.index, size,
                               dst.device, stream, default_copy_tuning(), up);
      return true;
    }
    *launched = pack_to_staging(src, dst.device, stream, staging, up);
    if (*launched != hipSuccess) return true;
    PullSrc staged;
    staged.same_proc = true;
    staged.buf.ptr = (uint8_t*)*staging;
    staged.buf.size = size;
    staged.buf.device = dst.device;
    // Dense source now: the next call launches at most one more kernel and
    // allocates no staging. An indexed source used `up` above, and then the
    // destination is rows or N-D and needs none; a rows or N-D source did
    // not, and the indexed destination takes it now.
    return copy_d2d(dst, staged, size, stream, staging, up, launched, err);
  }
  // Pull engine selection: gfx950 copy kernel (default) or the SDMA
  // engines via hipMemcpyPeerAsync/hipMemcpyAsync (STARWAY_PULL=sdma).
  // SDMA leaves CUs free and can ride dedicated copy engines; the kernel
  // streams a large same-device message at 6.4 TB/s of HBM traffic
  // (docs/benchmark.md "Streaming copy") and is the measured-fast default.
  static const bool use_sdma = [] {
    const char* v = getenv("STARWAY_PULL");
    return v && strcmp(v, "sdma") == 0;
  }();
  if (src.nd.ndim > 0 || dst.nd.ndim > 0) {
    // The only geometry requirement is the total size (check_window).
    Layout sl{}, dl{};
    try {
      sl = layout_of(src, size);
      dl = layout_of(dst, size);
    } catch (const std::invalid_argument& ex) {
      *err = ex.what();
      return false;
    }
    *launched = launch_copy_nd(dst.ptr, dl, src.ptr, sl, size, stream);
  } else if (src.rows > 0 || dst.rows > 0) {
    // Pack/unpack inside the pull kernel. Row geometry: the source's if it
    // has one; a rows destination must agree with it. (The N-D kernel
    // could serve two rows sides that differ; that is not done.)
    const BufferRef& g = src.rows > 0 ? src : dst;
    if (dst.rows > 0 && (dst.rows != g.rows || dst.row_bytes != g.row_bytes)) {
      *err = "strided send/recv row geometry mismatch";
      return false;
    }
    *launched = launch_copy_strided(
        dst.ptr, dst.rows > 0 ? dst.stride : g.row_bytes, src.ptr,
        src.rows > 0 ? src.stride : g.row_bytes, g.rows, g.row_bytes, stream);
  } else if (use_sdma) {
    if (from.same_proc && src.device != dst.device)
      *launched = hipMemcpyPeerAsync(dst.ptr, dst.device, src.ptr, src.device,
                                     size, stream);
    else
      *launched = hipMemcpyAsync(dst.ptr, src.ptr, size,
                                 hipMemcpyDeviceToDevice, stream);
  } else {
    // A source on another GPU is an xGMI pull and keeps the grid-stride
    // kernels: the streaming route was measured same-device only.
    *launched = launch_copy(dst.ptr, src.ptr, size, stream,
                            src.device == dst.device);
  }
  return true;
}

// Routes, by destination:
//   host      download(): D2H copy, 2-D copy for a rows source, N-D source
//             packed into device staging first
//   reducing  accumulate(): k_accum_* from the source where it lies, or
//             from staging (rows, N-D, element-misaligned source)
//   converting  accumulate() as well, ending in k_convert_*; on lane 0
//             only when it also reduces
//   device    copy_d2d(): one copy kernel (or SDMA) per geometry pair
void* begin_pull(const RtsDesc& rts, const IndexRef& src_index,
                 const BufferRef& dst, uint64_t size, std::string* err) {
  RoctxSpan span("starway::pull");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available in receiver process";
    return nullptr;
  }
  // The device whose context performs the copy: the destination device for
  // device recv buffers, else the sender's device ordinal (same node).
  const int run_dev = dst.device >= 0 ? dst.device : rts.device;
  PullSrc src;
  if (!decode_rts(rts, src_index, size, run_dev, &src, err)) return nullptr;

  DeviceGuard on(run_dev);
  // Lane by SOURCE DEVICE: on a real one-process-per-GPU topology the 7
  // peers live on 7 distinct devices => distinct lanes, full overlap
  // across xGMI links. Same-device peers (shared-GPU emulation) share a
  // lane, which also keeps the per-device HSA queue count low there.
  // Every accumulate into one device rides ONE stream, lane 0 (begin_h2d's
  // too), not the per-source-device lane: two read-modify-write kernels on
  // one buffer must never overlap, and any number of reducing receives
  // into the same buffer may be in flight, from any mix of peers.
  const int lane = dst.reducing() ? 0 : rts.device & (stream_lanes() - 1);
  hipStream_t stream = pull_stream(run_dev, lane);
  hipError_t e = hipSuccess;
  void* staging = nullptr;
  IndexUpload up;
  if (dst.device < 0) {
    e = download(dst.ptr, src.buf, run_dev, stream, &staging, &up);
  } else {
    if (src.same_proc) ensure_peer_access(dst.device, rts.device);
    log_route_once(run_dev, rts, src.same_proc, lane,
                   dst.converting() ? "gfx950_convert"
                   : dst.reducing() ? "gfx950_accum"
                                    : "gfx950_copy");
    if (dst.reducing() || dst.converting()) {
      if (!check_reduce_dst(dst, size, err)) return nullptr;
      e = accumulate(dst, src.buf, run_dev, stream, &staging, &up);
    } else {
      if (!check_window(dst, size, err)) return nullptr;
      if (!copy_d2d(dst, src, size, stream, &staging, &up, &e, err)) {
        // A pair refused after the source was packed: nothing may leak.
        abandon_route(staging, &up, stream);
        return nullptr;
      }
    }
  }
  return finish_ticket(run_dev, stream, staging, &up, e, "pull launch",
                       "event", err);
}

void* begin_pull_multi(const PullReq* reqs, int n, std::string* err) {
  RoctxSpan span("starway::pull_multi");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available in receiver process";
    return nullptr;
  }
  if (n < 1 || n > kMultiMax) {
    *err = "begin_pull_multi: bad batch size";
    return nullptr;
  }
  int run_dev = reqs[0].dst_device;
  MultiCopyDesc descs[kMultiMax];
  for (int i = 0; i < n; i++) {
    PullSrc src;
    if (!decode_rts(reqs[i].rts, IndexRef{}, reqs[i].size, run_dev, &src,
                    err))
      return nullptr;
    if (src.same_proc) ensure_peer_access(run_dev, reqs[i].rts.device);
    log_route_once(run_dev, reqs[i].rts, src.same_proc, 0, "gfx950_multi");
    descs[i] = {src.buf.ptr, reqs[i].dst_ptr, (uint32_t)reqs[i].size};
  }
  DeviceGuard on(run_dev);
  hipStream_t stream = pull_stream(run_dev, 0);
  hipError_t e = launch_copy_multi(descs, n, stream);
  return finish_ticket(run_dev, stream, nullptr, nullptr, e, "multi pull",
                       "multi pull", err);
}

void* begin_h2d(const BufferRef& dst, const void* src, uint64_t size,
                std::string* err) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available for device recv buffer";
    return nullptr;
  }
  DeviceGuard on(dst.device);
  // pull_stream(device) is lane 0: the one stream all accumulates into
  // this device share (see begin_pull).
  hipStream_t stream = pull_stream(dst.device);
  hipError_t e = hipSuccess;
  void* staging = nullptr;
  IndexUpload up;
  if (dst.reducing() || dst.converting()) {
    if (!check_reduce_dst(dst, size, err)) return nullptr;
    if (size > 0) {
      e = stage_from_host(src, size, stream, &staging);
      if (e == hipSuccess) e = launch_typed(dst, staging, size, stream);
    }
  } else if (!check_window(dst, size, err)) {
    return nullptr;
  } else if (dst.index.on()) {
    // Host -> staging -> k_copy_indexed -> destination.
    e = stage_from_host(src, size, stream, &staging);
    if (e == hipSuccess)
      e = copy_indexed(dst.ptr, dst.index, staging, IndexRef{}, size,
                       dst.device, stream, default_copy_tuning(), &up);
  } else if (dst.nd.ndim > 0) {
    // hipMemcpy2DAsync cannot express an N-D layout: host -> staging ->
    // k_copy_nd -> destination.
    e = stage_from_host(src, size, stream, &staging);
    if (e == hipSuccess)
      e = launch_copy_nd(dst.ptr, dst.nd, staging, contiguous_layout(size),
                         size, stream);
  } else if (dst.rows > 0) {
    e = hipMemcpy2DAsync(dst.ptr, dst.stride, src, dst.row_bytes,
                         dst.row_bytes, dst.rows, hipMemcpyHostToDevice,
                         stream);
  } else {
    e = hipMemcpyAsync(dst.ptr, src, size, hipMemcpyHostToDevice, stream);
  }
  return finish_ticket(dst.device, stream, staging, &up, e, "h2d",
                       "h2d", err);
}

void* begin_d2h(void* host_dst, const BufferRef& src, std::string* err) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available";
    return nullptr;
  }
  DeviceGuard on(src.device);
  hipStream_t stream = pull_stream(src.device);
  void* staging = nullptr;
  IndexUpload up;
  hipError_t e = download(host_dst, src, src.device, stream, &staging, &up);
  return finish_ticket(src.device, stream, staging, &up, e, "d2h",
                       "d2h", err);
}

void attach_bounce(void* ticket, RawBuf&& bounce) {
  ((Ticket*)ticket)->bounce = std::move(bounce);
}

int poll_ticket(void* ticket, std::string* err) {
  Ticket* t = (Ticket*)ticket;
  hipError_t e = hipEventQuery(t->ev);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  *err = hip_error("copy failed", e);
  return -1;
}

void free_ticket(void* ticket) {
  Ticket* t = (Ticket*)ticket;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    // A ticket freed before its event has passed (a canceled receive) may
    // leave its kernel reading the index buffer: not pooled then.
    if (t->index.dev)
      index_buf_put(&t->index, t->ev && hipEventQuery(t->ev) == hipSuccess);
    if (t->ev) pool_put_event(t->device, t->ev);
  }
  if (t->dev_staging) hipFree(t->dev_staging);
  delete t;
}

// ---------------------------------------------------------------------------
// Test/bench hooks: synchronous launches of the copy kernels on the pull
// stream, optionally with an explicit tuning (0 in a field = the default).
// ---------------------------------------------------------------------------

CopyTuning copy_tuning() { return default_copy_tuning(); }

static CopyTuning resolve_tuning(const CopyTuning& t) {
  CopyTuning r = default_copy_tuning();
  if (t.block_cap) r.block_cap = t.block_cap;
  if (t.nt_threshold) r.nt_threshold = t.nt_threshold;
  if (t.nt_unroll) r.nt_unroll = t.nt_unroll;
  if (t.stream_threshold) r.stream_threshold = t.stream_threshold;
  if (t.stream_blocks) r.stream_blocks = t.stream_blocks;
  if (t.accum_nt_threshold) r.accum_nt_threshold = t.accum_nt_threshold;
  return r;
}

int copy_stream_unroll() { return sw::copy_stream_unroll(); }

// Take g_mu, switch to `device`, run `launch` on its pull stream and wait.
template <class Launch>
static bool run_sync(int device, std::string* err, Launch launch) {
  if (!available()) {
    *err = "no HIP device";
    return false;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard on(device);
  hipStream_t stream = pull_stream(device);
  hipError_t e = launch(stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    *err = hipGetErrorString(e);
    return false;
  }
  return true;
}

bool copy_device_sync(void* dst, const void* src, size_t n, int device,
                      const CopyTuning& tuning, std::string* err) {
  CopyTuning t = resolve_tuning(tuning);
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_tuned(dst, src, n, stream, t);
  });
}

bool copy_strided_sync(void* dst, uint64_t dst_stride, const void* src,
                       uint64_t src_stride, uint64_t rows, uint64_t row_bytes,
                       int device, size_t block_cap, std::string* err) {
  CopyTuning t = resolve_tuning(CopyTuning{.block_cap = block_cap});
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_strided(dst, dst_stride, src, src_stride, rows,
                                     row_bytes, stream, t);
  });
}

bool copy_nd_sync(void* dst, const Layout& dst_layout, const void* src,
                  const Layout& src_layout, uint64_t bytes, int device,
                  size_t block_cap, CopyNdPath path, IndexWidth width,
                  bool* ineligible, std::string* err) {
  CopyTuning t = resolve_tuning(CopyTuning{.block_cap = block_cap});
  *ineligible = path == CopyNdPath::Tiled &&
                !copy_nd_tile_eligible(src_layout, dst_layout, src, dst);
  if (*ineligible) {
    *err = "the tiled kernel does not serve this pair of layouts";
    return false;
  }
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_nd(dst, dst_layout, src, src_layout, bytes,
                                stream, t, path, width);
  });
}

int copy_nd_tile_extent(int elem_bytes) {
  return sw::copy_nd_tile_extent(elem_bytes);
}

bool copy_index_sync(void* dst, const IndexRef& dst_index, const void* src,
                     const IndexRef& src_index, uint64_t bytes, int device,
                     size_t block_cap, IndexWidth width, std::string* err) {
  CopyTuning t = resolve_tuning(CopyTuning{.block_cap = block_cap});
  IndexUpload up;
  const bool ok = run_sync(device, err, [&](hipStream_t stream) {
    return copy_indexed(dst, dst_index, src, src_index, bytes, device, stream,
                        t, &up, width);
  });
  if (up.dev) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceGuard on(device);
    index_buf_put(&up, ok);
  }
  return ok;
}

bool accum_sync(void* dst, const void* src, size_t nbytes, ElemType dtype,
                int device, const CopyTuning& tuning, std::string* err) {
  const size_t es = elem_size(dtype);
  if (es == 0 || nbytes % es || ((uintptr_t)dst | (uintptr_t)src) % es) {
    *err = "pointers and length must be multiples of the element size";
    return false;
  }
  CopyTuning t = resolve_tuning(tuning);
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_accum(dst, src, nbytes, dtype, stream, t);
  });
}

bool convert_sync(void* dst, ElemType dst_type, const void* src,
                  ElemType src_type, size_t n_elems, bool accumulate,
                  int device, const CopyTuning& tuning, std::string* err) {
  CopyTuning t = resolve_tuning(tuning);
  t.convert_shape = tuning.convert_shape;
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_convert(dst, dst_type, src, src_type, n_elems, accumulate,
                          stream, t);
  });
}

ConvertPlan convert_plan(uintptr_t dst, ElemType dst_type, uintptr_t src,
                         ElemType src_type, size_t n_elems,
                         ConvertShape shape) {
  return sw::convert_plan(dst, dst_type, src, src_type, n_elems, shape);
}

ConvertShape convert_default_shape() { return sw::convert_default_shape(); }
void set_convert_default_shape(ConvertShape shape) {
  sw::set_convert_default_shape(shape);
}

// Callers validate 1 <= n <= kMultiMax and bytes < 2^32 (launch_copy_multi does not).
bool copy_multi_sync(const CopyDesc* descs, int n, int device,
                     std::string* err) {
  if (n < 1 || n > kMultiMax) {
    *err = "copy_multi_sync: bad batch size";
    return false;
  }
  MultiCopyDesc d[kMultiMax];
  for (int i = 0; i < n; i++)
    d[i] = {(const uint8_t*)descs[i].src, (uint8_t*)descs[i].dst,
            (uint32_t)descs[i].bytes};
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_multi(d, n, stream);
  });
}

void synchronize_all() {
  if (!available()) return;
  std::lock_guard<std::mutex> lk(g_mu);
  int n = cached_device_count();
  for (int d = 0; d < n; d++) {
    DeviceGuard on(d);
    for (int lane = 0; lane < stream_lanes(); lane++)
      if (hipStream_t s = pull_stream(d, lane)) hipStreamSynchronize(s);
  }
}

}  // namespace gpu
}  // namespace sw
