// device_util.h -- the few device / host helpers that ba.hip and band_solve.hip share.  Internal linkage, like se3_device.h:
// every translation unit that includes it gets its own copy (and its own per-device caches).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double d2a_t __attribute__((ext_vector_type(2), aligned(16)));

// the wave's index in its workgroup as a SCALAR: branches on it are scalar branches (derived from threadIdx.x alone the
// compiler treats it as divergent and wraps every wave-specialised region in exec-mask saves and restores)
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// One value per device, made on first use under a lock.  get(): the current device's, or `unavailable` if that device
// cannot be told.  make(dev) runs while the slot holds T{}: returning T{} on failure means "ask again next time".
template <typename T>
struct PerDevice {
  std::mutex mu;
  T slot[64] = {};
  template <typename Make>
  T get(T unavailable, Make make) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return unavailable;
    std::lock_guard<std::mutex> lock(mu);
    if (!slot[dev]) slot[dev] = make(dev);
    return slot[dev];
  }
};

// compute units of the current device (cached per device)
int device_cu_count() {
  static PerDevice<int> cached;
  return cached.get(0, [](int dev) {
    int n_cu = 0;
    return hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? n_cu : 0;
  });
}

}  // namespace
