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

#include <dlfcn.h>
#include <sys/stat.h>
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cstring>
#include <tuple>

namespace sw {
// kernels.hip
struct MultiCopyDesc {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t bytes;
};
hipError_t launch_copy_multi(const MultiCopyDesc* descs, int n,
                             hipStream_t stream);
// same_device: src and dst live on the GPU that runs the kernel. Only then
// may the copy take the streaming route (see launch_copy in kernels.hip).
hipError_t launch_copy(void* dst, const void* src, size_t bytes,
                       hipStream_t stream, bool same_device);
int copy_stream_unroll();
hipError_t launch_copy_strided(void* dst, uint64_t dst_stride,
                               const void* src, uint64_t src_stride,
                               uint64_t rows, uint64_t row_bytes,
                               hipStream_t stream);
hipError_t launch_copy_tuned(void* dst, const void* src, size_t bytes,
                             hipStream_t stream, const CopyTuning& t);
hipError_t launch_copy_strided_tuned(void* dst, uint64_t dst_stride,
                                     const void* src, uint64_t src_stride,
                                     uint64_t rows, uint64_t row_bytes,
                                     hipStream_t stream, const CopyTuning& t);
hipError_t launch_copy_nd(void* dst, const Layout& dst_layout,
                          const void* src, const Layout& src_layout,
                          uint64_t bytes, hipStream_t stream);
hipError_t launch_copy_nd_tuned(void* dst, const Layout& dst_layout,
                                const void* src, const Layout& src_layout,
                                uint64_t bytes, hipStream_t stream,
                                const CopyTuning& t, CopyNdPath path);
int copy_nd_tile_extent(int elem_bytes);
// dst[i] += src[i]; both pointers aligned to the element size, bytes a
// multiple of it, no overlap.
hipError_t launch_accum(void* dst, const void* src, size_t bytes,
                        ElemType dtype, hipStream_t stream);
hipError_t launch_accum_tuned(void* dst, const void* src, size_t bytes,
                              ElemType dtype, hipStream_t stream,
                              const CopyTuning& t);
bool copy_nd_tile_eligible(const Layout& src_layout, const Layout& dst_layout,
                           const void* src, const void* dst);

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

// Timed device copy through the production kernel: dst/src on (possibly
// different) devices, kernel runs on dst_dev (the pull pattern).
static double timed_copy_gbps(int dst_dev, int src_dev, size_t nbytes) {
  int prev;
  hipGetDevice(&prev);
  void* src = nullptr;
  void* dst = nullptr;
  hipSetDevice(src_dev);
  if (hipMalloc(&src, nbytes) != hipSuccess) {
    hipSetDevice(prev);
    return 0;
  }
  hipMemset(src, 1, nbytes);
  hipSetDevice(dst_dev);
  if (hipMalloc(&dst, nbytes) != hipSuccess) {
    hipSetDevice(src_dev);
    hipFree(src);
    hipSetDevice(prev);
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
  hipSetDevice(src_dev);
  hipFree(src);
  hipSetDevice(prev);
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
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(device);
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
    s = nullptr;
  hipSetDevice(prev);
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
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(dst_dev);
  hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
  (void)e;  // hipErrorPeerAccessAlreadyEnabled is fine
  hipSetDevice(prev);
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

void ipc_close_all() {
  std::lock_guard<std::mutex> lk0(g_mu);
  std::lock_guard<std::mutex> lk(g_ipc_mu);
  int prev = 0;
  hipGetDevice(&prev);
  for (auto& [key, base] : g_import_cache) {
    hipSetDevice(key.first);
    hipIpcCloseMemHandle(base);
  }
  hipSetDevice(prev);
  g_import_cache.clear();
  g_export_cache.clear();
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
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(buf.device);
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
  hipSetDevice(prev);
  // use_ipc==0 is still fine for same-process delivery (raw_ptr path);
  // a cross-process receiver will report the error.
  return true;
}

// ---------------------------------------------------------------------------
// tickets
// ---------------------------------------------------------------------------

struct Ticket {
  hipEvent_t ev = nullptr;
  int device = -1;
  RawBuf bounce;  // host staging kept alive until completion
  // Contiguous device staging of an N-D host<->device transfer; released
  // with the ticket.
  void* dev_staging = nullptr;
};

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

// The source side of a pull as a Layout, checked against the message size
// (the descriptor comes from the peer).
static bool rts_layout(const RtsDesc& rts, uint64_t size, Layout* out,
                       std::string* err) {
  try {
    if (rts.src_nd.ndim > 0) {
      *out = rts.src_nd;
      if (out->ndim > kMaxDims || out->unit == 0 ||
          layout_bytes(*out) != size) {
        *err = "malformed N-D source layout in RTS";
        return false;
      }
    } else if (rts.src_rows > 0) {
      *out = rows_layout(rts.src_rows, rts.src_row_bytes, rts.src_stride);
    } else {
      *out = contiguous_layout(size);
    }
  } catch (const std::invalid_argument& e) {
    *err = e.what();
    return false;
  }
  return true;
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
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(open_device);
  hipError_t e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
  hipSetDevice(prev);
  if (e != hipSuccess) {
    *err = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e);
    return nullptr;
  }
  g_import_cache[ck] = base;
  return base;
}

static void* resolve_src(const RtsDesc& rts, int open_device,
                         std::string* err) {
  bool same_proc = memcmp(rts.src_uuid, process_uuid(), 16) == 0;
  if (same_proc) return (void*)(uintptr_t)rts.raw_ptr;
  if (!rts.use_ipc) {
    *err = "peer did not export an IPC handle (cross-process GPU transfer)";
    return nullptr;
  }
  void* base = import_ipc(rts.ipc_handle, open_device, err);
  if (!base) return nullptr;
  return (uint8_t*)base + rts.offset;
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

void* begin_pull(const RtsDesc& rts, const BufferRef& dst, uint64_t size,
                 std::string* err) {
  RoctxSpan span("starway::pull");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available in receiver process";
    return nullptr;
  }
  // The device whose context performs the copy: the destination device for
  // device recv buffers, else the sender's device ordinal (same node).
  int run_dev = dst.device >= 0 ? dst.device : rts.device;
  void* src = resolve_src(rts, run_dev, err);
  if (!src) return nullptr;

  int prev;
  hipGetDevice(&prev);
  hipSetDevice(run_dev);
  // Lane by SOURCE DEVICE: on a real one-process-per-GPU topology the 7
  // peers live on 7 distinct devices => distinct lanes, full overlap
  // across xGMI links. Same-device peers (shared-GPU emulation) share a
  // lane, which also keeps the per-device HSA queue count low there.
  int lane = rts.device & (stream_lanes() - 1);
  // Every accumulate into one device rides ONE stream, lane 0 (begin_h2d's
  // too), not the per-source-device lane: two read-modify-write kernels on
  // one buffer must never overlap, and any number of reducing receives
  // into the same buffer may be in flight, from any mix of peers.
  if (dst.reducing()) lane = 0;
  hipStream_t stream = pull_stream(run_dev, lane);
  hipError_t e;
  void* staging = nullptr;
  if (dst.device >= 0 && dst.reducing()) {
    bool same_proc = memcmp(rts.src_uuid, process_uuid(), 16) == 0;
    if (same_proc) ensure_peer_access(dst.device, rts.device);
    log_route_once(run_dev, rts, same_proc, lane, "gfx950_accum");
    const size_t es = elem_size(dst.elem);
    if (!dst.dense() || es == 0 || (uintptr_t)dst.ptr % es || size % es ||
        size > dst.size) {
      hipSetDevice(prev);
      *err = "reduce: destination or message length does not fit the "
             "element type";
      return nullptr;
    }
    const bool packed = rts.src_rows == 0 && rts.src_nd.ndim == 0;
    if (packed && (uintptr_t)src % es == 0) {
      // Fast route: the accumulate kernel reads the source where it lies
      // (peer memory over xGMI, hipIpc-mapped, or local).
      e = launch_accum(dst.ptr, src, size, dst.elem, stream);
    } else {
      // Slow route (rows, N-D or element-misaligned source): pack into
      // contiguous device staging with the copy kernels, then accumulate
      // from staging; same stream, so in order.
      // Staging holds `size` bytes: the peer's geometry must describe
      // exactly that many.
      Layout sl{};
      if (rts.src_nd.ndim > 0 && !rts_layout(rts, size, &sl, err)) {
        hipSetDevice(prev);
        return nullptr;
      }
      if (rts.src_rows > 0 && rts.src_rows * rts.src_row_bytes != size) {
        hipSetDevice(prev);
        *err = "malformed strided source layout in RTS";
        return nullptr;
      }
      e = alloc_staging(size, &staging);
      if (e == hipSuccess) {
        if (rts.src_nd.ndim > 0)
          e = launch_copy_nd(staging, contiguous_layout(size), src, sl, size,
                             stream);
        else if (rts.src_rows > 0)
          e = launch_copy_strided(staging, rts.src_row_bytes, src,
                                  rts.src_stride, rts.src_rows,
                                  rts.src_row_bytes, stream);
        else
          e = launch_copy(staging, src, size, stream,
                          rts.device == run_dev);
      }
      if (e == hipSuccess)
        e = launch_accum(dst.ptr, staging, size, dst.elem, stream);
    }
  } else if (dst.device >= 0) {
    bool same_proc = memcmp(rts.src_uuid, process_uuid(), 16) == 0;
    if (same_proc) ensure_peer_access(dst.device, rts.device);
    log_route_once(run_dev, rts, same_proc, lane, "gfx950_copy");
    // Pull engine selection: gfx950 copy kernel (default) or the SDMA
    // engines via hipMemcpyPeerAsync/hipMemcpyAsync (STARWAY_PULL=sdma).
    // SDMA leaves CUs free and can ride dedicated copy engines; the kernel
    // streams a large same-device message at 6.4 TB/s of HBM traffic
    // (docs/benchmark.md "Streaming copy") and is the measured-fast default.
    static const bool use_sdma = [] {
      const char* v = getenv("STARWAY_PULL");
      return v && strcmp(v, "sdma") == 0;
    }();
    bool src_strided = rts.src_rows > 0;
    bool dst_strided = dst.rows > 0;
    const bool nd = rts.src_nd.ndim > 0 || dst.nd.ndim > 0;
    if (!dst.dense() && dst.size != size) {
      hipSetDevice(prev);
      *err = "strided recv buffer geometry mismatch (buffer " +
             std::to_string(dst.size) + " B, message " +
             std::to_string(size) + " B)";
      return nullptr;
    }
    if (nd) {
      // Either side N-D: both are expressed as layouts, and the only
      // geometry requirement is the total size (checked above).
      Layout sl{}, dl{};
      bool ok = rts_layout(rts, size, &sl, err);
      try {
        if (ok) dl = dst.dense() ? contiguous_layout(size) : dst.layout();
      } catch (const std::invalid_argument& ex) {
        *err = ex.what();
        ok = false;
      }
      if (!ok) {
        hipSetDevice(prev);
        return nullptr;
      }
      e = launch_copy_nd(dst.ptr, dl, src, sl, size, stream);
    } else if (src_strided || dst_strided) {
      // Pack/unpack inside the pull kernel. Row geometry: prefer the
      // source's; a strided dst must agree on row_bytes.
      uint64_t rows = src_strided ? rts.src_rows : dst.rows;
      uint64_t row_bytes = src_strided ? rts.src_row_bytes : dst.row_bytes;
      if (dst_strided && src_strided &&
          (dst.rows != rows || dst.row_bytes != row_bytes)) {
        hipSetDevice(prev);
        *err = "strided send/recv row geometry mismatch";
        return nullptr;
      }
      uint64_t sstride = src_strided ? rts.src_stride : row_bytes;
      uint64_t dstride = dst_strided ? dst.stride : row_bytes;
      e = launch_copy_strided(dst.ptr, dstride, src, sstride, rows,
                              row_bytes, stream);
    } else if (use_sdma) {
      if (same_proc && rts.device != dst.device) {
        e = hipMemcpyPeerAsync(dst.ptr, dst.device, src, rts.device, size,
                               stream);
      } else {
        e = hipMemcpyAsync(dst.ptr, src, size, hipMemcpyDeviceToDevice,
                           stream);
      }
    } else {
      // A source on another GPU (rts.device != run_dev) is an xGMI pull and
      // keeps the grid-stride kernels: the streaming route was measured
      // same-device only.
      e = launch_copy(dst.ptr, src, size, stream, rts.device == run_dev);
    }
  } else {
    if (rts.src_nd.ndim > 0) {
      Layout sl{};
      if (!rts_layout(rts, size, &sl, err)) {
        hipSetDevice(prev);
        return nullptr;
      }
      e = alloc_staging(size, &staging);
      if (e == hipSuccess)
        e = launch_copy_nd(staging, contiguous_layout(size), src, sl, size,
                           stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(dst.ptr, staging, size, hipMemcpyDeviceToHost,
                           stream);
    } else if (rts.src_rows > 0) {
      e = hipMemcpy2DAsync(dst.ptr, rts.src_row_bytes, src, rts.src_stride,
                           rts.src_row_bytes, rts.src_rows,
                           hipMemcpyDeviceToHost, stream);
    } else {
      e = hipMemcpyAsync(dst.ptr, src, size, hipMemcpyDeviceToHost, stream);
    }
  }
  if (e != hipSuccess) {
    drop_staging(staging, stream);
    hipSetDevice(prev);
    *err = std::string("pull launch: ") + hipGetErrorString(e);
    return nullptr;
  }
  Ticket* t = new Ticket();
  t->device = run_dev;
  t->dev_staging = staging;
  e = pool_get_event(run_dev, &t->ev);
  if (e == hipSuccess) e = hipEventRecord(t->ev, stream);
  hipSetDevice(prev);
  if (e != hipSuccess) {
    *err = std::string("event: ") + hipGetErrorString(e);
    drop_staging(staging, stream);
    delete t;
    return nullptr;
  }
  return t;
}

void* begin_pull_multi(const PullReq* reqs, int n, std::string* err) {
  RoctxSpan span("starway::pull_multi");
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available in receiver process";
    return nullptr;
  }
  if (n < 1 || n > 8) {
    *err = "begin_pull_multi: bad batch size";
    return nullptr;
  }
  int run_dev = reqs[0].dst_device;
  MultiCopyDesc descs[8];
  for (int i = 0; i < n; i++) {
    void* src = resolve_src(reqs[i].rts, run_dev, err);
    if (!src) return nullptr;
    bool same_proc =
        memcmp(reqs[i].rts.src_uuid, process_uuid(), 16) == 0;
    if (same_proc) ensure_peer_access(run_dev, reqs[i].rts.device);
    log_route_once(run_dev, reqs[i].rts, same_proc, 0, "gfx950_multi");
    descs[i] = {(const uint8_t*)src, reqs[i].dst_ptr,
                (uint32_t)reqs[i].size};
  }
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(run_dev);
  hipStream_t stream = pull_stream(run_dev, 0);
  hipError_t e = launch_copy_multi(descs, n, stream);
  Ticket* t = nullptr;
  if (e == hipSuccess) {
    t = new Ticket();
    t->device = run_dev;
    e = pool_get_event(run_dev, &t->ev);
    if (e == hipSuccess) e = hipEventRecord(t->ev, stream);
  }
  hipSetDevice(prev);
  if (e != hipSuccess) {
    *err = std::string("multi pull: ") + hipGetErrorString(e);
    delete t;
    return nullptr;
  }
  return t;
}

void* begin_h2d(const BufferRef& dst, const void* src, uint64_t size,
                std::string* err) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available for device recv buffer";
    return nullptr;
  }
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(dst.device);
  hipStream_t stream = pull_stream(dst.device);
  hipError_t e;
  void* staging = nullptr;
  if (dst.reducing()) {
    // pull_stream(device) is lane 0: the one stream all accumulates into
    // this device share (see begin_pull).
    const size_t es = elem_size(dst.elem);
    if (!dst.dense() || es == 0 || (uintptr_t)dst.ptr % es || size % es ||
        size > dst.size) {
      hipSetDevice(prev);
      *err = "reduce: destination or message length does not fit the "
             "element type";
      return nullptr;
    }
    e = hipSuccess;
    if (size > 0) {
      e = alloc_staging(size, &staging);
      if (e == hipSuccess)
        e = hipMemcpyAsync(staging, src, size, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess)
        e = launch_accum(dst.ptr, staging, size, dst.elem, stream);
    }
  } else if (dst.nd.ndim > 0) {
    if (size != dst.size) {
      hipSetDevice(prev);
      *err = "strided recv buffer geometry mismatch (buffer " +
             std::to_string(dst.size) + " B, message " +
             std::to_string(size) + " B)";
      return nullptr;
    }
    e = alloc_staging(size, &staging);
    if (e == hipSuccess)
      e = hipMemcpyAsync(staging, src, size, hipMemcpyHostToDevice, stream);
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
  Ticket* t = nullptr;
  if (e == hipSuccess) {
    t = new Ticket();
    t->device = dst.device;
    e = pool_get_event(dst.device, &t->ev);
    if (e == hipSuccess) e = hipEventRecord(t->ev, stream);
  }
  if (e == hipSuccess) t->dev_staging = staging;
  else drop_staging(staging, stream);
  hipSetDevice(prev);
  if (e != hipSuccess) {
    *err = std::string("h2d: ") + hipGetErrorString(e);
    delete t;
    return nullptr;
  }
  return t;
}

void* begin_d2h(void* host_dst, const BufferRef& src, std::string* err) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!available()) {
    *err = "no HIP device available";
    return nullptr;
  }
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(src.device);
  hipStream_t stream = pull_stream(src.device);
  hipError_t e;
  void* staging = nullptr;
  if (src.nd.ndim > 0) {
    e = alloc_staging(src.size, &staging);
    if (e == hipSuccess)
      e = launch_copy_nd(staging, contiguous_layout(src.size), src.ptr,
                         src.nd, src.size, stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(host_dst, staging, src.size, hipMemcpyDeviceToHost,
                         stream);
  } else if (src.rows > 0) {
    e = hipMemcpy2DAsync(host_dst, src.row_bytes, src.ptr, src.stride,
                         src.row_bytes, src.rows, hipMemcpyDeviceToHost,
                         stream);
  } else {
    e = hipMemcpyAsync(host_dst, src.ptr, src.size, hipMemcpyDeviceToHost,
                       stream);
  }
  Ticket* t = nullptr;
  if (e == hipSuccess) {
    t = new Ticket();
    t->device = src.device;
    e = pool_get_event(src.device, &t->ev);
    if (e == hipSuccess) e = hipEventRecord(t->ev, stream);
  }
  if (e == hipSuccess) t->dev_staging = staging;
  else drop_staging(staging, stream);
  hipSetDevice(prev);
  if (e != hipSuccess) {
    *err = std::string("d2h: ") + hipGetErrorString(e);
    delete t;
    return nullptr;
  }
  return t;
}

void attach_bounce(void* ticket, RawBuf&& bounce) {
  ((Ticket*)ticket)->bounce = std::move(bounce);
}

int poll_ticket(void* ticket, std::string* err) {
  Ticket* t = (Ticket*)ticket;
  hipError_t e = hipEventQuery(t->ev);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  *err = std::string("copy failed: ") + hipGetErrorString(e);
  return -1;
}

void free_ticket(void* ticket) {
  Ticket* t = (Ticket*)ticket;
  if (t->ev) {
    std::lock_guard<std::mutex> lk(g_mu);
    pool_put_event(t->device, t->ev);
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
  int prev;
  hipGetDevice(&prev);
  hipSetDevice(device);
  hipStream_t stream = pull_stream(device);
  hipError_t e = launch(stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  hipSetDevice(prev);
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
  CopyTuning t = resolve_tuning(CopyTuning{block_cap, 0, 0});
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_strided_tuned(dst, dst_stride, src, src_stride, rows,
                                     row_bytes, stream, t);
  });
}

bool copy_nd_sync(void* dst, const Layout& dst_layout, const void* src,
                  const Layout& src_layout, uint64_t bytes, int device,
                  size_t block_cap, CopyNdPath path, bool* ineligible,
                  std::string* err) {
  CopyTuning t = resolve_tuning(CopyTuning{block_cap, 0, 0});
  *ineligible = path == CopyNdPath::Tiled &&
                !copy_nd_tile_eligible(src_layout, dst_layout, src, dst);
  if (*ineligible) {
    *err = "the tiled kernel does not serve this pair of layouts";
    return false;
  }
  return run_sync(device, err, [&](hipStream_t stream) {
    return launch_copy_nd_tuned(dst, dst_layout, src, src_layout, bytes,
                                stream, t, path);
  });
}

int copy_nd_tile_extent(int elem_bytes) {
  return sw::copy_nd_tile_extent(elem_bytes);
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
    return launch_accum_tuned(dst, src, nbytes, dtype, stream, t);
  });
}

// Callers validate 1 <= n <= 8 and bytes < 2^32 (launch_copy_multi does not).
bool copy_multi_sync(const CopyDesc* descs, int n, int device,
                     std::string* err) {
  if (n < 1 || n > 8) {
    *err = "copy_multi_sync: bad batch size";
    return false;
  }
  MultiCopyDesc d[8];
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
  int prev;
  hipGetDevice(&prev);
  for (int d = 0; d < n; d++) {
    for (int lane = 0; lane < stream_lanes(); lane++) {
      hipStream_t s = pull_stream(d, lane);
      if (s) {
        hipSetDevice(d);
        hipStreamSynchronize(s);
      }
    }
  }
  hipSetDevice(prev);
}

}  // namespace gpu
}  // namespace sw
