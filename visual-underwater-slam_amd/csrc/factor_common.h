// factor_common.h -- what the add-on factor families (between.hip, point_prior.hip, pose_meas.hip) share besides the SE(3) and
// robust-loss arithmetic of se3_device.h: the workgroup's error partial, the guarded CSR row lookup, and the host-side
// read-back and validation of a factor set.  sym3 is also used by ba.hip and marginals.hip.  Internal linkage, like
// se3_device.h and device_util.h: every translation unit that includes it gets its own copy.
#pragma once
#include <cmath>
#include <vector>
#include "vus_common.h"

namespace {

// ---- device ---------------------------------------------------------------------------------------------------------
// the workgroup's sum of `e` (0 for a thread without a row) in a fixed tree order, written by thread 0 to part[block].
// Two uses in one kernel share the LDS tree: the caller puts a __syncthreads() between them.
template <int WG>
__device__ __forceinline__ void block_partial(double e, double* __restrict__ part) {
  __shared__ double s[WG];
  s[threadIdx.x] = e;
  __syncthreads();
#pragma unroll
  for (int o = WG / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// row r of a CSR over n factors: its item i (a landmark or a pose, of n_items) and factor range [a, b); false for a row a
// checked factor set cannot hold (check_csr_rows refuses it), which then reads and writes nothing.  The struct's fields
// come by reference: each is read where it is used, behind the guards before it, as when this stood in the kernels'
// own units (by value they are all read first, and the kernels come out with other instructions).
__device__ __forceinline__ bool csr_row(const int& n_rows, const int* const& row_item, const int* const& row_ptr,
                                        const int& n_items, const int& n, int r, int& i, int& a, int& b) {
  if (r >= n_rows) return false;
  i = row_item[r];
  a = row_ptr[r];
  b = row_ptr[r + 1];
  return (unsigned)i < (unsigned)n_items && a >= 0 && a <= b && b <= n;
}

// entry (r, c) of a symmetric 3 x 3 in upper-triangle storage xx, xy, xz, yy, yz, zz
__device__ __forceinline__ double sym3(const double* v, int r, int c) {
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return v[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
}

// ---- host -----------------------------------------------------------------------------------------------------------
template <typename T>
int read_back(const T* src, size_t n, std::vector<T>& dst, hipStream_t st) {
  dst.resize(n);
  if (n == 0) return VUS_OK;
  VUS_CHECK_HIP(hipMemcpyAsync(dst.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost, st));
  VUS_CHECK_HIP(hipStreamSynchronize(st));
  return VUS_OK;
}

// n == 0: the sums are 0 and nothing is launched
int zero_out(double* out, int count, hipStream_t st) {
  VUS_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(double) * count, st));
  return VUS_OK;
}

// the CSR rows of a factor set, read back: row_ptr runs 0..n, and per row its item in range, strictly ascending, and the
// row non-empty.  `row_name` is the array ("row_pose"), `item` the noun ("pose") of the messages.
int check_csr_rows(const std::vector<int>& rows, const std::vector<int>& ptr, int n_rows, int n, int n_items, const char* row_name,
                   const char* item) {
  VUS_REQUIRE(ptr[0] == 0 && ptr[n_rows] == n, "row_ptr runs from %d to %d, not from 0 to n=%d", ptr[0], ptr[n_rows], n);
  for (int r = 0; r < n_rows; ++r) {
    VUS_REQUIRE(rows[r] >= 0 && rows[r] < n_items, "row %d: %s %d outside [0, %d)", r, item, rows[r], n_items);
    VUS_REQUIRE(r == 0 || rows[r] > rows[r - 1], "%s is not strictly ascending at row %d (%d after %d)", row_name, r, rows[r],
                r ? rows[r - 1] : 0);
    VUS_REQUIRE(ptr[r + 1] > ptr[r], "row %d (%s %d) is empty or row_ptr decreases (%d, %d)", r, item, rows[r], ptr[r], ptr[r + 1]);
  }
  return VUS_OK;
}

// factor f's own robust model (include/vus_robust.h): a known kind, and k finite and > 0 unless Gaussian
int check_factor_loss(int f, int kind, double k) {
  VUS_REQUIRE(kind >= VUS_LOSS_GAUSSIAN && kind <= VUS_LOSS_WELSCH, "factor %d: unknown loss kind %d", f, kind);
  VUS_REQUIRE(kind == VUS_LOSS_GAUSSIAN || (k > 0.0 && std::isfinite(k)), "factor %d: loss parameter k=%g must be finite and > 0", f, k);
  return VUS_OK;
}

// one whitening weight (1 / sigma) of factor f
int check_factor_weight(int f, double w) {
  VUS_REQUIRE(std::isfinite(w) && w > 0.0, "factor %d: weight w=%g must be finite and > 0", f, w);
  return VUS_OK;
}

}  // namespace
