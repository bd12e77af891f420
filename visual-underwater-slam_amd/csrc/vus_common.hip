// vus_common.hip -- error reporting, the fixed-order sum and the version entry points of libvus_hip.so.
#include "vus_common.h"
#include <cstdarg>

namespace vus {

char* last_error_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

}  // namespace vus

namespace {
// out[0] = sum of part[0..n) in a fixed order (one workgroup)
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const double* __restrict__ part, int n,
                                                               double* __restrict__ out) {
  __shared__ double s[1024];
  double acc = 0;
  for (int k = threadIdx.x; k < n; k += 1024) acc += part[k];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s[0];
}
}  // namespace

// the one host launcher of the fixed-order sum (called from ba.hip, nav.hip and between.hip)
void vus::reduce_partials(const double* part, int n, double* out, hipStream_t st) {
  reduce_partials_kernel<<<1, 1024, 0, st>>>(part, n, out);
}

extern "C" int vus_abi_version(void) { return VUS_ABI_VERSION; }
extern "C" const char* vus_last_error(void) { return vus::last_error_buf(); }
#ifndef VUS_OFFLOAD_TARGET
#define VUS_OFFLOAD_TARGET "unknown"
#endif
extern "C" const char* vus_build_target(void) { return VUS_OFFLOAD_TARGET; }
