// Standalone copy-kernel microbench (no Python/torch): the measuring tool
// for the copy kernels, and the rocprofv3 PMC target (tracing the full
// Python process has been seen to crash the profiler).
//
//   copy_bench [bytes] [iters]              one variant ("prod"), one line
//   copy_bench --size B --iters N --rounds R --variants a,b,c
//              [--stream-blocks S] [--pairs P]
//
// Variants: prod (launch_copy, the production route), old_nt4, old_nt8,
// old_plain (the grid-stride kernels, through launch_copy_tuned), and every
// streaming instantiation stream_u{4,8}_{nn,pn,pp}_{np,pf}: U, cache policy
// (nn = nt loads + nt stores, pn = plain loads + nt stores, pp = plain +
// plain), prefetch off/on. "all" names every variant; --list prints them.
//
// The source holds a position-dependent pattern; each variant copies it
// once into a poisoned destination and the WHOLE destination plus a guard
// band behind it is verified on the GPU before the variant is timed. A
// variant that fails is reported and not timed. Timing is hipEvent around
// `iters` back-to-back launches that rotate over P (>= 4) distinct
// source/destination pairs, so the footprint is well past the 256 MiB
// Infinity Cache. With several variants the rounds alternate: round r times
// every variant once, in order, and every round is printed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "copy_stream.hpp"
#include "kernels.hpp"

#define CHECK(x)                                                    \
  do {                                                              \
    hipError_t e_ = (x);                                            \
    if (e_ != hipSuccess) {                                         \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_)); \
      return 1;                                                     \
    }                                                               \
  } while (0)

namespace {

constexpr size_t kGuardBytes = 4096;
constexpr unsigned kPoison = 0xEE;

// 16 B element i of pair `salt`: every element differs from its neighbours
// and from the same position one tile, one grid stride or 2^32 elements on.
__device__ __forceinline__ uint4 pattern(uint64_t i, uint32_t salt) {
  const uint32_t lo = (uint32_t)i, hi = (uint32_t)(i >> 32);
  return make_uint4(lo, hi ^ salt, lo * 2654435761u + salt, ~lo ^ (hi << 7));
}

__global__ __launch_bounds__(256) void k_fill_pattern(uint4* buf, uint64_t n16,
                                                      uint32_t salt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += stride)
    buf[i] = pattern(i, salt);
}

// Counts wrong elements in [0, n16) and changed guard elements behind them.
__global__ __launch_bounds__(256) void k_verify(const uint4* buf, uint64_t n16,
                                                uint64_t guard16,
                                                uint32_t salt,
                                                unsigned long long* bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t p = kPoison * 0x01010101u;
  unsigned long long mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n16 + guard16; i += stride) {
    const uint4 got = buf[i];
    const uint4 want = i < n16 ? pattern(i, salt) : make_uint4(p, p, p, p);
    if (got.x != want.x || got.y != want.y || got.z != want.z ||
        got.w != want.w)
      mine++;
  }
  if (mine) atomicAdd(bad, mine);
}

struct Variant {
  std::string name;
  // Launch over `bytes` (a multiple of 16, 16 B-aligned pointers).
  hipError_t (*launch)(void* dst, const void* src, size_t bytes,
                       size_t stream_blocks, hipStream_t stream);
};

hipError_t run_prod(void* d, const void* s, size_t n, size_t, hipStream_t st) {
  return sw::launch_copy(d, s, n, st, true);
}
template <int UNROLL, bool NT>
hipError_t run_old(void* d, const void* s, size_t n, size_t, hipStream_t st) {
  sw::CopyTuning t = sw::default_copy_tuning();
  t.nt_threshold = NT ? 1 : sw::kStreamNever;
  t.nt_unroll = UNROLL;
  t.stream_threshold = sw::kStreamNever;
  return sw::launch_copy_tuned(d, s, n, st, t);
}
template <int U, int POLICY, bool PF>
hipError_t run_stream(void* d, const void* s, size_t n, size_t stream_blocks,
                      hipStream_t st) {
  return sw::launch_copy_stream<U, POLICY, PF>(d, s, n / 16, stream_blocks,
                                               st);
}

template <int U, int POLICY>
void add_stream(std::vector<Variant>* v, const char* pol) {
  const std::string base = "stream_u" + std::to_string(U) + "_" + pol;
  v->push_back({base + "_np", run_stream<U, POLICY, false>});
  v->push_back({base + "_pf", run_stream<U, POLICY, true>});
}

std::vector<Variant> all_variants() {
  std::vector<Variant> v;
  v.push_back({"prod", run_prod});
  v.push_back({"old_nt4", run_old<4, true>});
  v.push_back({"old_nt8", run_old<8, true>});
  v.push_back({"old_plain", run_old<4, false>});
  add_stream<4, sw::kStreamNtNt>(&v, "nn");
  add_stream<4, sw::kStreamPlainNt>(&v, "pn");
  add_stream<4, sw::kStreamPlainPlain>(&v, "pp");
  add_stream<8, sw::kStreamNtNt>(&v, "nn");
  add_stream<8, sw::kStreamPlainNt>(&v, "pn");
  add_stream<8, sw::kStreamPlainPlain>(&v, "pp");
  return v;
}

int grid_for(uint64_t n16) {
  return (int)std::min<uint64_t>((n16 + 255) / 256, 8192);
}

}  // namespace

int main(int argc, char** argv) {
  size_t bytes = 256ull << 20;
  int iters = 10, rounds = 1, pairs = 4;
  size_t stream_blocks = 0;  // 0: the process default
  std::string want = "prod";
  bool legacy = true;  // positional [bytes] [iters]: one summary line
  int npos = 0;
  const std::vector<Variant> all = all_variants();
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* {
      if (i + 1 >= argc) {
        fprintf(stderr, "%s needs a value\n", a.c_str());
        exit(2);
      }
      return argv[++i];
    };
    if (a == "--list") {
      for (const Variant& v : all) printf("%s\n", v.name.c_str());
      return 0;
    } else if (a == "--size") {
      bytes = strtoull(val(), nullptr, 10), legacy = false;
    } else if (a == "--iters") {
      iters = atoi(val()), legacy = false;
    } else if (a == "--rounds") {
      rounds = atoi(val()), legacy = false;
    } else if (a == "--pairs") {
      pairs = atoi(val()), legacy = false;
    } else if (a == "--stream-blocks") {
      stream_blocks = strtoull(val(), nullptr, 10), legacy = false;
    } else if (a == "--variants") {
      want = val(), legacy = false;
    } else if (a.rfind("--", 0) == 0) {
      fprintf(stderr, "unknown flag %s\n", a.c_str());
      return 2;
    } else if (npos == 0) {
      bytes = strtoull(a.c_str(), nullptr, 10), npos++;
    } else if (npos == 1) {
      iters = atoi(a.c_str()), npos++;
    } else {
      fprintf(stderr, "unexpected argument %s\n", a.c_str());
      return 2;
    }
  }
  bytes &= ~(size_t)15;  // whole 16 B elements: the bulk the kernels serve
  if (bytes == 0 || iters < 1 || rounds < 1 || pairs < 1) {
    fprintf(stderr, "need bytes >= 16, iters, rounds, pairs >= 1\n");
    return 2;
  }
  if (stream_blocks == 0) stream_blocks = sw::default_copy_tuning().stream_blocks;
  if (stream_blocks == 0) stream_blocks = 1;

  std::vector<Variant> sel;
  if (want == "all") {
    sel = all;
  } else {
    size_t pos = 0;
    while (pos <= want.size()) {
      size_t comma = want.find(',', pos);
      if (comma == std::string::npos) comma = want.size();
      const std::string name = want.substr(pos, comma - pos);
      pos = comma + 1;
      if (name.empty()) continue;
      auto it = std::find_if(all.begin(), all.end(),
                             [&](const Variant& v) { return v.name == name; });
      if (it == all.end()) {
        fprintf(stderr, "unknown variant %s (see --list)\n", name.c_str());
        return 2;
      }
      sel.push_back(*it);
    }
  }
  if (sel.empty()) {
    fprintf(stderr, "no variant selected\n");
    return 2;
  }

  const uint64_t n16 = bytes / 16, guard16 = kGuardBytes / 16;
  std::vector<void*> src(pairs), dst(pairs);
  hipStream_t stream;
  CHECK(hipStreamCreate(&stream));
  for (int p = 0; p < pairs; p++) {
    CHECK(hipMalloc(&src[p], bytes));
    CHECK(hipMalloc(&dst[p], bytes + kGuardBytes));
    hipLaunchKernelGGL(k_fill_pattern, dim3(grid_for(n16)), dim3(256), 0,
                       stream, (uint4*)src[p], n16, (uint32_t)p);
    CHECK(hipGetLastError());
  }
  unsigned long long* bad;
  CHECK(hipMalloc(&bad, sizeof(*bad)));
  CHECK(hipStreamSynchronize(stream));

  // Verify each variant on every pair (this also warms it up); a failing
  // variant is reported and dropped.
  std::vector<Variant> ok;
  for (const Variant& v : sel) {
    unsigned long long total_bad = 0;
    for (int p = 0; p < pairs; p++) {
      CHECK(hipMemsetAsync(dst[p], kPoison, bytes + kGuardBytes, stream));
      CHECK(hipMemsetAsync(bad, 0, sizeof(*bad), stream));
      CHECK(v.launch(dst[p], src[p], bytes, stream_blocks, stream));
      hipLaunchKernelGGL(k_verify, dim3(grid_for(n16 + guard16)), dim3(256),
                         0, stream, (const uint4*)dst[p], n16, guard16,
                         (uint32_t)p, bad);
      CHECK(hipGetLastError());
      unsigned long long h = 0;
      CHECK(hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost,
                           stream));
      CHECK(hipStreamSynchronize(stream));
      total_bad += h;
    }
    if (total_bad) {
      printf("VERIFY FAIL variant=%s size=%zu stream_blocks=%zu: %llu wrong "
             "16B elements; not timed\n",
             v.name.c_str(), bytes, stream_blocks, total_bad);
    } else {
      ok.push_back(v);
    }
  }
  fflush(stdout);

  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  std::vector<std::vector<double>> us(ok.size());
  for (int r = 0; r < rounds; r++) {
    for (size_t k = 0; k < ok.size(); k++) {
      CHECK(hipEventRecord(t0, stream));
      for (int i = 0; i < iters; i++)
        CHECK(ok[k].launch(dst[i % pairs], src[i % pairs], bytes,
                           stream_blocks, stream));
      CHECK(hipEventRecord(t1, stream));
      CHECK(hipStreamSynchronize(stream));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, t0, t1));
      const double s = ms / 1e3 / iters;
      us[k].push_back(s * 1e6);
      if (legacy) {
        printf("%zu bytes: %.3f TB/s payload (%.3f TB/s HBM traffic), "
               "%.1f us\n",
               bytes, bytes / s / 1e12, 2 * bytes / s / 1e12, s * 1e6);
      } else {
        printf("round=%d variant=%s size=%zu stream_blocks=%zu iters=%d "
               "pairs=%d us=%.2f hbm_tbps=%.3f\n",
               r, ok[k].name.c_str(), bytes, stream_blocks, iters, pairs,
               s * 1e6, 2 * bytes / s / 1e12);
      }
    }
  }
  if (!legacy) {
    for (size_t k = 0; k < ok.size(); k++) {
      std::vector<double> v = us[k];
      std::sort(v.begin(), v.end());
      printf("summary variant=%s size=%zu stream_blocks=%zu rounds=%d "
             "min_us=%.2f median_us=%.2f max_us=%.2f\n",
             ok[k].name.c_str(), bytes, stream_blocks, rounds, v.front(),
             v[v.size() / 2], v.back());
    }
  }
  return ok.size() == sel.size() ? 0 : 1;
}
