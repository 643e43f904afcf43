// device_guard.h -- every C ABI entry point works on the decoder's device and puts the caller's current device back on exit (a process
// that uses several GPUs must not find PyTorch's current device switched by a decode -- or by a destructor that the garbage collector
// runs at an arbitrary time).  Host code; included by the .hip files that hold entry points.
#pragma once
#include <hip/hip_runtime.h>

namespace ctcdev {

struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  DeviceGuard() = default;  // (no device yet: enter() follows)
  explicit DeviceGuard(int dev) { (void)enter(dev); }
  hipError_t enter(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur;
    if (cur != dev) err = hipSetDevice(dev);
    return err;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

}  // namespace ctcdev
