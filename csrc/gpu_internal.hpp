// Shared by the two translation units of the GPU layer, gpu.cpp and
// smallmsg.hip. Nothing else belongs here: each keeps its own mutex, stream
// map and event pool (ROUND2_NOTES.md, hardware-queue starvation).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace sw {
namespace gpu {

// Scoped device switch. These functions run on the engine's progress thread
// and on Python threads alike; a switch that is not undone leaves the thread
// on the wrong device for the rest of the process, so hipSetDevice is
// called here and nowhere else in the GPU layer.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    (void)hipGetDevice(&prev_);
    status_ = hipSetDevice(device);
  }
  ~DeviceGuard() { (void)hipSetDevice(prev_); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  // Whether the switch succeeded (the destructor restores either way).
  bool ok() const { return status_ == hipSuccess; }
  hipError_t status() const { return status_; }

 private:
  int prev_ = 0;
  hipError_t status_ = hipSuccess;
};

// "what: <HIP's text for e>", the form of every error string of the layer.
inline std::string hip_error(const char* what, hipError_t e) {
  return std::string(what) + ": " + hipGetErrorString(e);
}

// Map a peer's exported allocation on open_device (cached per device x
// handle; gpu.cpp). Shared by the pull path and the inbox push path.
void* import_ipc(const uint8_t* handle, int open_device, std::string* err);

}  // namespace gpu
}  // namespace sw
