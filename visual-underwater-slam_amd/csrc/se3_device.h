// se3_device.h -- device helpers shared by the pose kernels of ba.hip, between.hip, pose_meas.hip and nav.hip: SE(3) in gtsam's
// Pose3 / Rot3 conventions (tangent order (omega, v), retract T * Exp(xi), local Log(T^-1 T2)), the flat12 pose load and the
// robust-loss table of include/vus_robust.h with its run-time dispatcher.  Internal linkage: every translation unit that
// includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vus.h"

namespace {

constexpr double kEps = 2.220446049250313e-16;

// a pose (flat12: R row-major, then t) into registers
__device__ __forceinline__ void load12(const double* __restrict__ src, double* dst) {
#pragma unroll
  for (int k = 0; k < 12; ++k) dst[k] = src[k];
}

// ---------------------------------------------------------------------------------------------
// Lie-group helpers (gtsam Pose3 / Rot3 conventions; mirrored independently by the CPU oracle)
__device__ void so3_expmap(const double* w, double* R) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double Wx[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  if (th2 <= kEps) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Wx[i] + (i % 4 == 0 ? 1.0 : 0.0);
    return;
  }
  const double th = sqrt(th2);
  const double s = sin(th) / th;
  const double sh = sin(0.5 * th);
  const double c = 2.0 * sh * sh / th2;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      double ww = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) ww += Wx[3 * r + k] * Wx[3 * k + cc];
      R[3 * r + cc] = (r == cc ? 1.0 : 0.0) + s * Wx[3 * r + cc] + c * ww;
    }
}

// Log of SO(3).  acos(cos th) and the division by sin th lose accuracy like eps / sin^2 th towards pi (3e-14 at 3.04 rad,
// 1e-5 at pi - 1e-5), so below tr = -0.4 (angles above 134 degrees, sin^2 th < 1/2) the angle comes from
// atan2(sin th, cos th) with sin th = |v| / 2, v the antisymmetric part, and the axis from the symmetric part
// (R + R^T) / 2 = cos th I + (1 - cos th) a a^T: the column of its largest diagonal entry, signed by v.  Accurate to a few
// eps up to pi itself (where the sign of the axis is arbitrary).  The branches for tr >= -0.4 are gtsam's SO3::Logmap
// (4.0/4.1 form) unchanged.
__device__ void so3_logmap(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  if (tr < -0.4) {
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double c = 0.5 * (tr - 1.0);
    const double th = atan2(0.5 * sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), c);
    const int i = R[0] >= R[4] ? (R[0] >= R[8] ? 0 : 2) : (R[4] >= R[8] ? 1 : 2);
    double a[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = 0.5 * (R[3 * j + i] + R[3 * i + j]) - (j == i ? c : 0.0);
    double k = th / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (v[0] * a[0] + v[1] * a[1] + v[2] * a[2] < 0.0) k = -k;
    w[0] = k * a[0]; w[1] = k * a[1]; w[2] = k * a[2];
    return;
  }
  double mag;
  const double tr3 = tr - 3.0;
  if (tr3 < -1e-7) {
    double th = acos((tr - 1.0) / 2.0);
    mag = th / (2.0 * sin(th));
  } else {
    mag = 0.5 - tr3 / 12.0;
  }
  w[0] = mag * (R[7] - R[5]);
  w[1] = mag * (R[2] - R[6]);
  w[2] = mag * (R[3] - R[1]);
}

// out = T * Exp(xi).  The translation of Exp is V v = v + b (w x v) + c (w x (w x v)), b = (1 - cos th) / th^2,
// c = (th - sin th) / th^3: summed in this form its error is a few eps |v| at every angle (the cancellation in c is
// scaled by th^2 |v|), where (I - R)(w x v) / th^2 loses eps |v| / th and the first-order Exp below kEps dropped b.
__device__ void pose_retract(const double* T, const double* xi, double* out) {
  double Re[9], te[3];
  so3_expmap(xi, Re);
  const double* w = xi;
  const double* v = xi + 3;
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double b = 0.5, c = 1.0 / 6.0;
  if (th2 > kEps) {
    const double th = sqrt(th2), sh = sin(0.5 * th);
    b = 2.0 * sh * sh / th2;
    c = (th - sin(th)) / (th2 * th);
  }
  const double wv[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};
  const double wwv[3] = {w[1] * wv[2] - w[2] * wv[1], w[2] * wv[0] - w[0] * wv[2], w[0] * wv[1] - w[1] * wv[0]};
#pragma unroll
  for (int r = 0; r < 3; ++r) te[r] = v[r] + b * wv[r] + c * wwv[r];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[3 * r + c] = T[3 * r] * Re[c] + T[3 * r + 1] * Re[3 + c] + T[3 * r + 2] * Re[6 + c];
    out[9 + r] = T[9 + r] + (T[3 * r] * te[0] + T[3 * r + 1] * te[1] + T[3 * r + 2] * te[2]);
  }
}

// xi = Logmap(T^-1 * T2)
__device__ void pose_local(const double* T, const double* T2, double* xi) {
  double R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = T[r] * T2[c] + T[3 + r] * T2[3 + c] + T[6 + r] * T2[6 + c];
    t[r] = T[r] * (T2[9] - T[9]) + T[3 + r] * (T2[10] - T[10]) + T[6 + r] * (T2[11] - T[11]);
  }
  double w[3];
  so3_logmap(R, w);
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
  if (th < 1e-10) {   // V^-1 t = t - w x t / 2 + O(th^2 |t|)
    xi[3] = t[0] - 0.5 * (w[1] * t[2] - w[2] * t[1]);
    xi[4] = t[1] - 0.5 * (w[2] * t[0] - w[0] * t[2]);
    xi[5] = t[2] - 0.5 * (w[0] * t[1] - w[1] * t[0]);
    return;
  }
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double WT[3] = {k[1] * t[2] - k[2] * t[1], k[2] * t[0] - k[0] * t[2], k[0] * t[1] - k[1] * t[0]};
  const double WWT[3] = {k[1] * WT[2] - k[2] * WT[1], k[2] * WT[0] - k[0] * WT[2], k[0] * WT[1] - k[1] * WT[0]};
  const double tn = tan(0.5 * th);
#pragma unroll
  for (int r = 0; r < 3; ++r) xi[3 + r] = t[r] - (0.5 * th) * WT[r] + (1.0 - th / (2.0 * tn)) * WWT[r];
}

// Robust noise model (include/vus_robust.h): weight w and loss rho of a stereo factor from its squared whitened
// residual norm d2 = d^2.  Every kernel that reweights a factor calls this on the same d2 expression, so W / V (lin_points),
// Hpp / gp (lin_poses) and the linear error (eval_points) describe one weighted system.
template <int LOSS>
__device__ __forceinline__ void robust_weight(double d2, double k, double& w, double& rho) {
  const double k2 = k * k;
  if (LOSS == VUS_LOSS_HUBER) {
    const double d = sqrt(d2);
    w = d <= k ? 1.0 : k / d;
    rho = d <= k ? 0.5 * d2 : k * d - 0.5 * k2;
  } else if (LOSS == VUS_LOSS_CAUCHY) {
    w = k2 / (k2 + d2);
    rho = 0.5 * k2 * log1p(d2 / k2);
  } else if (LOSS == VUS_LOSS_TUKEY) {
    const double t = 1.0 - d2 / k2;
    w = d2 <= k2 ? t * t : 0.0;
    rho = d2 <= k2 ? (k2 / 6.0) * (1.0 - t * t * t) : k2 / 6.0;
  } else if (LOSS == VUS_LOSS_GEMAN_MCCLURE) {
    const double s = k2 + d2;
    w = (k2 * k2) / (s * s);
    rho = 0.5 * k2 * d2 / s;
  } else if (LOSS == VUS_LOSS_WELSCH) {
    w = exp(-d2 / k2);
    rho = -0.5 * k2 * expm1(-d2 / k2);
  } else {
    w = 1.0;
    rho = 0.5 * d2;
  }
}

// w and rho of factor f's own robust model, chosen at run time from the per-factor arrays of a factor set (a kind out of
// range reads as Gaussian; the set's vus_*_check refuses it)
__device__ __forceinline__ void robust_weight_of(const int* loss_kind, const double* loss_k, int f, double d2, double& w,
                                                 double& rho) {
  const double k = loss_k[f];
  switch (loss_kind[f]) {
    case VUS_LOSS_HUBER: robust_weight<VUS_LOSS_HUBER>(d2, k, w, rho); break;
    case VUS_LOSS_CAUCHY: robust_weight<VUS_LOSS_CAUCHY>(d2, k, w, rho); break;
    case VUS_LOSS_TUKEY: robust_weight<VUS_LOSS_TUKEY>(d2, k, w, rho); break;
    case VUS_LOSS_GEMAN_MCCLURE: robust_weight<VUS_LOSS_GEMAN_MCCLURE>(d2, k, w, rho); break;
    case VUS_LOSS_WELSCH: robust_weight<VUS_LOSS_WELSCH>(d2, k, w, rho); break;
    default: robust_weight<VUS_LOSS_GAUSSIAN>(d2, k, w, rho); break;
  }
}

}  // namespace
