// imu_device.h -- the ImuFactor arithmetic on the device, one copy for every unit that evaluates it (nav.hip: ImuFactor in
// both node layouts; combined_imu.hip: rows 0..8 of CombinedImuFactor): the offsets of the 148-double preintegration
// record, small 3 x 3 products, the SO(3) Jacobians and the factor's residual and Jacobian.  Internal linkage, like
// se3_device.h: every translation unit that includes it gets its own copy.
#pragma once
#include <cmath>
#include "se3_device.h"   // so3_expmap / so3_logmap: one copy for every pose kernel

namespace {

// ---- device math: SO(3) helpers and the ImuFactor residual / Jacobian --------------------------------------------------
constexpr int PIM_DT = 0, PIM_DR = 1, PIM_DP = 10, PIM_DV = 13, PIM_DR_DBG = 16, PIM_DP_DBA = 25, PIM_DP_DBG = 34,
              PIM_DV_DBA = 43, PIM_DV_DBG = 52, PIM_BIAS = 61, PIM_N = 148;

__device__ __forceinline__ void skew(const double* w, double* S) {
  S[0] = 0; S[1] = -w[2]; S[2] = w[1]; S[3] = w[2]; S[4] = 0; S[5] = -w[0]; S[6] = -w[1]; S[7] = w[0]; S[8] = 0;
}
__device__ __forceinline__ void mm(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mtm(const double* A, const double* B, double* C) {   // A^T B
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
__device__ __forceinline__ void mv(const double* A, const double* v, double* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
__device__ __forceinline__ void mtv(const double* A, const double* v, double* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = A[r] * v[0] + A[3 + r] * v[1] + A[6 + r] * v[2];
}

__device__ void so3_jr(const double* w, double* J) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9], WW[9];
  skew(w, W); mm(W, W, WW);
  double a, b;
  if (th2 < 1e-10) { a = 0.5 - th2 / 24.0; b = 1.0 / 6.0 - th2 / 120.0; }
  else {   // 1 - cos th as 2 sin^2(th / 2): its cancellation cost eps / th in a W (2e-11 at th = 1e-5)
    const double th = sqrt(th2), sh = sin(0.5 * th);
    a = 2.0 * sh * sh / th2; b = (th - sin(th)) / (th2 * th);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0 ? 1.0 : 0.0) - a * W[i] + b * WW[i];
}
__device__ void so3_jr_inv(const double* w, double* J) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9], WW[9];
  skew(w, W); mm(W, W, WW);
  double b;
  if (th2 < 1e-10) b = 1.0 / 12.0 + th2 / 720.0;
  else {   // (1 + cos th) / sin th as 1 / tan(th / 2): the quotient lost eps / sin th towards pi
    const double th = sqrt(th2);
    b = 1.0 / th2 - 1.0 / (2.0 * th * tan(0.5 * th));
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0 ? 1.0 : 0.0) + 0.5 * W[i] + b * WW[i];
}

// ImuFactor: unwhitened residual r[9] = (theta, p, v) and, when J != nullptr, the Jacobian J[9][24] with
// columns pose_i(6) vel_i(3) pose_j(6) vel_j(3) bias(6).  Forster et al. 2017 / gtsam ImuFactor.
__device__ void imu_factor(const double* Ti, const double* vi, const double* Tj, const double* vj, const double* bias,
                           const double* pim, const double* g, double* r, double* J) {
  const double dt = pim[PIM_DT];
  double dba[3], dbg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { dba[k] = bias[k] - pim[PIM_BIAS + k]; dbg[k] = bias[3 + k] - pim[PIM_BIAS + 3 + k]; }
  double phi[3], Ephi[9], dRc[9], dPc[3], dVc[3], t3[3], t3b[3];
  mv(pim + PIM_DR_DBG, dbg, phi);
  so3_expmap(phi, Ephi);
  mm(pim + PIM_DR, Ephi, dRc);
  mv(pim + PIM_DP_DBA, dba, t3); mv(pim + PIM_DP_DBG, dbg, t3b);
#pragma unroll
  for (int k = 0; k < 3; ++k) dPc[k] = pim[PIM_DP + k] + t3[k] + t3b[k];
  mv(pim + PIM_DV_DBA, dba, t3); mv(pim + PIM_DV_DBG, dbg, t3b);
#pragma unroll
  for (int k = 0; k < 3; ++k) dVc[k] = pim[PIM_DV + k] + t3[k] + t3b[k];
  const double* Ri = Ti; const double* pi = Ti + 9;
  const double* Rj = Tj; const double* pj = Tj + 9;
  double RjtRi[9], E[9], rR[3];
  mtm(Rj, Ri, RjtRi);
  mm(RjtRi, dRc, E);
  so3_logmap(E, rR);
  double RidP[3], RidV[3], dpw[3], dvw[3], rP[3], rV[3];
  mv(Ri, dPc, RidP); mv(Ri, dVc, RidV);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dpw[k] = pi[k] + vi[k] * dt + 0.5 * g[k] * dt * dt + RidP[k] - pj[k];
    dvw[k] = vi[k] + g[k] * dt + RidV[k] - vj[k];
  }
  mtv(Rj, dpw, rP); mtv(Rj, dvw, rV);
#pragma unroll
  for (int k = 0; k < 3; ++k) { r[k] = rR[k]; r[3 + k] = rP[k]; r[6 + k] = rV[k]; }
  if (!J) return;
  for (int k = 0; k < 9 * 24; ++k) J[k] = 0.0;
  double JrInv[9], JrInvNeg[9], M[9], M2[9], X[9], JrPhi[9];
  const double nrR[3] = {-rR[0], -rR[1], -rR[2]};
  so3_jr_inv(rR, JrInv);
  so3_jr_inv(nrR, JrInvNeg);
#define JSET(row0, col0, Mat, sgn)                                                         \
  for (int a = 0; a < 3; ++a)                                                              \
    for (int b = 0; b < 3; ++b) J[24 * ((row0) + a) + (col0) + b] = (sgn) * (Mat)[3 * a + b]
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) M[3 * a + b] = dRc[3 * b + a];
  mm(JrInv, M, M2);
  JSET(0, 0, M2, 1.0);
  JSET(0, 9, JrInvNeg, -1.0);
  so3_jr(phi, JrPhi);
  mm(JrInv, JrPhi, M); mm(M, pim + PIM_DR_DBG, M2);
  JSET(0, 21, M2, 1.0);
  skew(dPc, X); mm(RjtRi, X, M);
  JSET(3, 0, M, -1.0);
  JSET(3, 3, RjtRi, 1.0);
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) M[3 * a + b] = Rj[3 * b + a] * dt;
  JSET(3, 6, M, 1.0);
  skew(rP, X);
  JSET(3, 9, X, 1.0);
  for (int a = 0; a < 3; ++a) J[24 * (3 + a) + 12 + a] = -1.0;
  mm(RjtRi, pim + PIM_DP_DBA, M); JSET(3, 18, M, 1.0);
  mm(RjtRi, pim + PIM_DP_DBG, M); JSET(3, 21, M, 1.0);
  skew(dVc, X); mm(RjtRi, X, M);
  JSET(6, 0, M, -1.0);
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) M[3 * a + b] = Rj[3 * b + a];
  JSET(6, 6, M, 1.0);
  skew(rV, X);
  JSET(6, 9, X, 1.0);
  JSET(6, 15, M, -1.0);
  mm(RjtRi, pim + PIM_DV_DBA, M); JSET(6, 18, M, 1.0);
  mm(RjtRi, pim + PIM_DV_DBG, M); JSET(6, 21, M, 1.0);
#undef JSET
}

}  // namespace
