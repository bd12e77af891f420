// between_device.h -- the arithmetic of one BetweenFactor<Pose3> (include/vus_between.h), shared by the kernels that add the
// factor's blocks to the band (between.hip) and those that keep a long closure as a low-rank term (closure.hip): residual,
// H1 and the squared whitened norm the robust weight is taken from.  Internal linkage, like se3_device.h.
#pragma once
#include "se3_device.h"
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

}  // namespace
