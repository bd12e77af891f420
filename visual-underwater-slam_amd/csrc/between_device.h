// between_device.h -- the arithmetic of one BetweenFactor<Pose3> (include/vus_between.h), shared by the kernels that add the
// factor's blocks to the band (between.hip) and those that keep a long closure as a low-rank term (closure.hip): residual,
// H1, the squared whitened norm the robust weight is taken from, and the whitening of a full-covariance model (load R,
// whiten a 6-vector, whiten a 6 x 6).  Internal linkage, like se3_device.h.
#pragma once
#include "se3_device.h"
#include "factor_common.h"
#include "../../include/vus_between.h"

namespace {

struct BetweenLin {
  double r[6];                // Log(meas^-1 T1^-1 T2), unwhitened
  double H1[36];              // -Ad(hx^-1), row-major
};

// residual and H1 of factor f at poses (H2 = I); with WITH_H = false only the residual
template <bool WITH_H>
__device__ __forceinline__ void between_factor(const vus_between_factors& B, const double* __restrict__ poses, int f,
                                               BetweenLin& L) {
  const int ps = B.pose_stride;
  double T1[12], T2[12], M[12], hx[12];
  load12(poses + 12 * (size_t)(B.node1[f] / ps), T1);
  load12(poses + 12 * (size_t)(B.node2[f] / ps), T2);
  load12(B.meas + 12 * (size_t)f, M);
  // hx = T1^-1 T2: R = R1^T R2, t = R1^T (t2 - t1)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) hx[3 * r + c] = T1[r] * T2[c] + T1[3 + r] * T2[3 + c] + T1[6 + r] * T2[6 + c];
    hx[9 + r] = T1[r] * (T2[9] - T1[9]) + T1[3 + r] * (T2[10] - T1[10]) + T1[6 + r] * (T2[11] - T1[11]);
  }
  pose_local(M, hx, L.r);
  if (!WITH_H) return;
  // -Ad(hx^-1) = [[-R^T, 0], [R^T [t]x, -R^T]]   (Ad(T) = [[R, 0], [[t]x R, R]] in the (omega, v) order)
  const double* R = hx;
  const double* t = hx + 9;
  const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double rt = R[3 * c + r];                     // (R^T)(r, c)
      L.H1[6 * r + c] = -rt;
      L.H1[6 * r + 3 + c] = 0.0;
      L.H1[6 * (3 + r) + 3 + c] = -rt;
      L.H1[6 * (3 + r) + c] = R[r] * tx[c] + R[3 + r] * tx[3 + c] + R[6 + r] * tx[6 + c];
    }
}

__device__ __forceinline__ double whitened_sq(const double* __restrict__ w, const double* r) {
  double d2 = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) d2 += (w[k] * r[k]) * (w[k] * r[k]);
  return d2;
}

// The full-covariance model of a factor (vus_between_factors.sqrt_info): the upper-triangular R with R^T R = cov^-1, its
// 21 entries on and above the diagonal packed row by row.  Both paths whiten with these three functions, every sum in
// ascending column order k = q .. 5.
struct SqrtInfo {
  double R[21];
  static __device__ __forceinline__ constexpr int at(int q, int k) { return 6 * q - q * (q - 1) / 2 + (k - q); }   // k >= q
};

__device__ __forceinline__ void load_sqrt_info(const vus_between_factors& B, int f, SqrtInfo& S) {
  const double* __restrict__ m = B.sqrt_info + 36 * (size_t)f;
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int k = q; k < 6; ++k) S.R[SqrtInfo::at(q, k)] = m[6 * q + k];
}

// out = s R v
__device__ __forceinline__ void whiten6(const SqrtInfo& S, double s, const double* v, double* out) {
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    double a = 0;
#pragma unroll
    for (int k = q; k < 6; ++k) a += S.R[SqrtInfo::at(q, k)] * v[k];
    out[q] = s * a;
  }
}

// out = s R H (6 x 6, row-major)
__device__ __forceinline__ void whiten66(const SqrtInfo& S, double s, const double* H, double* out) {
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double a = 0;
#pragma unroll
      for (int k = q; k < 6; ++k) a += S.R[SqrtInfo::at(q, k)] * H[6 * k + c];
      out[6 * q + c] = s * a;
    }
}

// |v|^2, the squared norm of a whitened 6-vector
__device__ __forceinline__ double norm_sq6(const double* v) {
  double d2 = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) d2 += v[k] * v[k];
  return d2;
}

// host: sqrt_info [n, 36] of a factor set read back (NULL: the diagonal model, nothing to check) -- what the kernels
// read of it, the entries on and above the diagonal, must be finite and the diagonal > 0
int check_sqrt_info(const double* sqrt_info, int n, hipStream_t st) {
  if (sqrt_info == nullptr) return VUS_OK;
  std::vector<double> R;
  if (int rc = read_back(sqrt_info, 36 * (size_t)n, R, st)) return rc;
  for (int f = 0; f < n; ++f)
    for (int q = 0; q < 6; ++q) {
      for (int k = q; k < 6; ++k)
        VUS_REQUIRE(std::isfinite(R[36 * (size_t)f + 6 * q + k]), "factor %d: sqrt_info(%d, %d)=%g is not finite", f, q, k,
                    R[36 * (size_t)f + 6 * q + k]);
      VUS_REQUIRE(R[36 * (size_t)f + 7 * q] > 0.0, "factor %d: sqrt_info(%d, %d)=%g on the diagonal must be > 0", f, q, q,
                  R[36 * (size_t)f + 7 * q]);
    }
  return VUS_OK;
}

}  // namespace
