// ba.hip -- stereo bundle-adjustment kernels for gfx950 (MI355X), fp64.
//
// What gtsam.LevenbergMarquardtOptimizer(graph, values, params).optimize() (reference batch.py:337)
// spends its time on for a graph of GenericStereoFactor3D factors (batch.py:300-305) with
// PriorFactorPose3 gauge priors (batch.py:281): per-factor residual/Jacobian evaluation, damped
// normal equations, landmark Schur complement, reduced camera solve, back-substitution, retraction
// and error evaluation.  The Levenberg-Marquardt control flow stays on the host (ba.py).
//
// Layout (include/vus.h): observations in L-order (point-major) and P-order (pose-major) with both
// permutations precomputed; the per-observation 6x3 product W in L-ORDER (round 4; rounds 1-3: P-order), so that a
// landmark's rows of an 8-pose tile are consecutive: the tile-pair Schur kernel reads runs of up to 8 rows, the
// linearisation writes and the back-substitution reads W as one stream (Y = W Vinv is formed on the fly).
//
// Kernel map.  Reductions are fixed-order wave / LDS / DPP sums.  The reduced camera system S dp = -gs is solved by the
// block-band Cholesky of band_solve.hip, which shares only device_util.h with this file.
//   lin_points   wave / point      r, H1, H2 -> W (L-order: streamed), V, gl, error partial
//   lin_poses    workgroup / pose  r, H1 (recomputed, never stored) -> Hpp, gp
//   priors       one lane          PriorFactorPose3 information / gradient / error
//   vinv (ymul)  thread / point, thread / obs   (V + lambda I)^-1  (Y = W Vinv only as an optional output)
//   schur_tiles  S = Hpp + lambda I - sum Y W^T and gs = gp - sum Y gl as a block-sparse GEMM on v_mfma_f64_16x16x4:
//                persistent workgroups, one 8 x 8-pose tile pair at a time, the landmarks seen from both tiles side by
//                side along K (vus_ba_tiles, built by pack.hip)
//   backsub      wave / point      dl = -Vinv (gl + sum W^T dp)
//   retract, eval_points, error_points; the fixed-order sum of their partials is vus::reduce_partials (vus_common.hip)
#include <cmath>
#include <type_traits>
#include "vus_common.h"
#include "device_util.h"
#include "se3_device.h"
#include "factor_common.h"

namespace {

struct Calib {
  double fx, fy, cx, cy, b, w;
};

__device__ __forceinline__ Calib load_calib(const double* K, double inv_sigma) {
  return Calib{K[0], K[1], K[3], K[4], K[5], inv_sigma};
}

// GenericStereoFactor3D: whitened residual and (optionally) Jacobians.
// gtsam StereoCamera::project2: q = R^T (p - t); z <= 0 -> cheirality: residual 2 fx, zero Jacobians.
template <bool WITH_H1, bool WITH_H2>
__device__ __forceinline__ void stereo_factor(const double* __restrict__ T, const double* __restrict__ p,
                                              const double* __restrict__ m, const Calib& K, double* r,
                                              double* H1, double* H2) {
  const double d0 = p[0] - T[9], d1 = p[1] - T[10], d2 = p[2] - T[11];
  const double x = T[0] * d0 + T[3] * d1 + T[6] * d2;
  const double y = T[1] * d0 + T[4] * d1 + T[7] * d2;
  const double z = T[2] * d0 + T[5] * d1 + T[8] * d2;
  if (z <= 0.0) {
    r[0] = r[1] = r[2] = 2.0 * K.fx * K.w;
    if (WITH_H1)
#pragma unroll
      for (int k = 0; k < 18; ++k) H1[k] = 0.0;
    if (WITH_H2)
#pragma unroll
      for (int k = 0; k < 9; ++k) H2[k] = 0.0;
    return;
  }
  const double d = 1.0 / z;
  r[0] = (K.cx + d * K.fx * x - m[0]) * K.w;
  r[1] = (K.cx + d * K.fx * (x - K.b) - m[1]) * K.w;
  r[2] = (K.cy + d * K.fy * y - m[2]) * K.w;
  if (!WITH_H1 && !WITH_H2) return;
  const double J[9] = {K.w * d * K.fx, 0.0, -K.w * d * d * K.fx * x,
                       K.w * d * K.fx, 0.0, -K.w * d * d * K.fx * (x - K.b),
                       0.0, K.w * d * K.fy, -K.w * d * d * K.fy * y};
  if (WITH_H2)
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        H2[3 * rr + c] = J[3 * rr] * T[3 * c] + J[3 * rr + 1] * T[3 * c + 1] + J[3 * rr + 2] * T[3 * c + 2];
  if (WITH_H1) {
    const double Q[9] = {0, -z, y, z, 0, -x, -y, x, 0};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        H1[6 * rr + c] = J[3 * rr] * Q[c] + J[3 * rr + 1] * Q[3 + c] + J[3 * rr + 2] * Q[6 + c];
        H1[6 * rr + 3 + c] = -J[3 * rr + c];
      }
  }
}

// Stereo and monocular projection factors side by side (include/vus_mono.h).  gtsam GenericProjectionFactor<Pose3,
// Point3, Cal3_S2>: q = R^T (p - t), u = cx + fx x/z + s y/z, v = cy + fy y/z, residual (u - m_u, v - m_v) / sigma; z <= 0 ->
// cheirality: residual 2 fx / sigma on both rows, zero Jacobians.  With d = 1/z the rows of d(u, v)/dq are
//   (fx d, s d, -d^2 (fx x + s y))   and   (0, fy d, -d^2 fy y),
// i.e. the stereo factor's uL and v rows with a skew term, and then H2 = J R^T, H1 = [J [q]x, -J] as there.  So ONE body
// serves both kinds per lane: the calibration (fx, fy, s, cx, cy, b, w) is selected by the observation's flag (s = b = 0
// for a stereo lane, whose terms in s are then exact zeros and change no bit), the three rows are formed once, and the uR
// row (slot 1) of a mono lane is zero in r, H1 and H2 -- it adds nothing to any product, d^2 or error.  A wave holding
// both kinds runs this body once, not a stereo and a mono body in turn; a mono lane pays for a row of zeros.
struct MixedCalib {
  double fx, fy, s, cx, cy, b, w;
};
struct MonoArg {
  const unsigned char* is_mono;      // [n_obs] L-order
  double fx, fy, s, cx, cy, w;
};
struct NoMono {};
template <bool MIXED>
using mono_arg_t = std::conditional_t<MIXED, MonoArg, NoMono>;

template <bool WITH_H1, bool WITH_H2>
__device__ __forceinline__ void mixed_factor(const double* __restrict__ T, const double* __restrict__ p,
                                             const double* __restrict__ m, const MixedCalib& K, bool mono, double* r,
                                             double* H1, double* H2) {
  const double d0 = p[0] - T[9], d1 = p[1] - T[10], d2 = p[2] - T[11];
  const double x = T[0] * d0 + T[3] * d1 + T[6] * d2;
  const double y = T[1] * d0 + T[4] * d1 + T[7] * d2;
  const double z = T[2] * d0 + T[5] * d1 + T[8] * d2;
  if (z <= 0.0) {
    r[0] = r[2] = 2.0 * K.fx * K.w;
    r[1] = mono ? 0.0 : r[0];
    if (WITH_H1)
#pragma unroll
      for (int k = 0; k < 18; ++k) H1[k] = 0.0;
    if (WITH_H2)
#pragma unroll
      for (int k = 0; k < 9; ++k) H2[k] = 0.0;
    return;
  }
  const double d = 1.0 / z;
  r[0] = (K.cx + d * K.fx * x + d * K.s * y - m[0]) * K.w;
  r[1] = mono ? 0.0 : (K.cx + d * K.fx * (x - K.b) - m[1]) * K.w;
  r[2] = (K.cy + d * K.fy * y - m[2]) * K.w;
  if (!WITH_H1 && !WITH_H2) return;
  const double J[9] = {K.w * d * K.fx, K.w * d * K.s, -K.w * d * d * K.fx * x - K.w * d * d * K.s * y,
                       mono ? 0.0 : K.w * d * K.fx, 0.0, mono ? 0.0 : -K.w * d * d * K.fx * (x - K.b),
                       0.0, K.w * d * K.fy, -K.w * d * d * K.fy * y};
  if (WITH_H2)
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        H2[3 * rr + c] = J[3 * rr] * T[3 * c] + J[3 * rr + 1] * T[3 * c + 1] + J[3 * rr + 2] * T[3 * c + 2];
  if (WITH_H1) {
    const double Q[9] = {0, -z, y, z, 0, -x, -y, x, 0};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        H1[6 * rr + c] = J[3 * rr] * Q[c] + J[3 * rr + 1] * Q[3 + c] + J[3 * rr + 2] * Q[6 + c];
        H1[6 * rr + 3 + c] = -J[3 * rr + c];
      }
  }
}

// observation a (L-order) at camera pose T and point p: the stereo factor, or in a mixed instance the form its flag names.
// The middle slot of a mono observation's measurement is not used (it may hold anything, NaN included).
template <bool WITH_H1, bool WITH_H2, typename MA>
__device__ __forceinline__ void obs_factor(const vus_ba_problem& P, const Calib& K, const MA& M, int a,
                                           const double* __restrict__ T, const double* __restrict__ p, double* r,
                                           double* H1, double* H2) {
  if constexpr (std::is_same_v<MA, MonoArg>) {
    const bool mono = M.is_mono[a] != 0;
    const double m1 = P.meas[3 * (size_t)a + 1];
    const double m[3] = {P.meas[3 * (size_t)a], mono ? 0.0 : m1, P.meas[3 * (size_t)a + 2]};
    const MixedCalib C = {mono ? M.fx : K.fx, mono ? M.fy : K.fy, mono ? M.s : 0.0, mono ? M.cx : K.cx,
                          mono ? M.cy : K.cy, mono ? 0.0 : K.b, mono ? M.w : K.w};
    mixed_factor<WITH_H1, WITH_H2>(T, p, m, C, mono, r, H1, H2);
  } else {
    const double m[3] = {P.meas[3 * (size_t)a], P.meas[3 * (size_t)a + 1], P.meas[3 * (size_t)a + 2]};
    stereo_factor<WITH_H1, WITH_H2>(T, p, m, K, r, H1, H2);
  }
}

__host__ __device__ __forceinline__ int pose_stride(const vus_ba_problem& P) { return P.pose_stride > 1 ? P.pose_stride : 1; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// body_P_sensor (include/vus_sensor.h): S and Ad(S^-1), made once on the host (make_sensor) and passed BY VALUE in the
// kernel arguments -- uniform across the launch, so scalar loads and no per-lane traffic.  The diagonal blocks of
// Ad(S^-1) are Rs^T, read out of T transposed (sensor_A) instead of being carried twice: 42 scalar registers, not 60.
// The instances without an extrinsic take the empty NoSensor in that place and are the kernels they were without it.
struct SensorArg {
  double T[12];     // S = (Rs row-major, ts)
  double B[9];      // -Rs^T [ts]x: the lower-left block of Ad(S^-1)
};
__device__ __forceinline__ double sensor_A(const SensorArg& S, int r, int c) { return S.T[3 * c + r]; }     // Rs^T
struct NoSensor {};
template <bool SENSOR>
using sensor_arg_t = std::conditional_t<SENSOR, SensorArg, NoSensor>;

// the camera pose of a keyframe: its 12 doubles, or with an extrinsic C = X o S = (Rb Rs, tb + Rb ts)
template <typename SA>
__device__ __forceinline__ void load_camera(const double* __restrict__ src, const SA& S, double* T) {
  if constexpr (std::is_same_v<SA, SensorArg>) {
    double X[12];
    load12(src, X);
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) T[3 * rr + c] = X[3 * rr] * S.T[c] + X[3 * rr + 1] * S.T[3 + c] + X[3 * rr + 2] * S.T[6 + c];
      T[9 + rr] = X[9 + rr] + (X[3 * rr] * S.T[9] + X[3 * rr + 1] * S.T[10] + X[3 * rr + 2] * S.T[11]);
    }
  } else {
    load12(src, T);
  }
}

// H1 (3 x 6, camera tangent [omega, v]) <- H1 Ad(S^-1) = [Hw A + Hv B, Hv A]: the Jacobian in the body tangent
template <typename SA>
__device__ __forceinline__ void h1_to_body(const SA& S, double* H1) {
  if constexpr (std::is_same_v<SA, SensorArg>) {
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      const double w0 = H1[6 * rr], w1 = H1[6 * rr + 1], w2 = H1[6 * rr + 2];
      const double v0 = H1[6 * rr + 3], v1 = H1[6 * rr + 4], v2 = H1[6 * rr + 5];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        H1[6 * rr + c] = (w0 * sensor_A(S, 0, c) + w1 * sensor_A(S, 1, c) + w2 * sensor_A(S, 2, c)) +
                         (v0 * S.B[c] + v1 * S.B[3 + c] + v2 * S.B[6 + c]);
        H1[6 * rr + 3 + c] = v0 * sensor_A(S, 0, c) + v1 * sensor_A(S, 1, c) + v2 * sensor_A(S, 2, c);
      }
    }
  }
}

// a body-tangent step as the camera's: d <- Ad(S^-1) d = [A w, B w + A v]  (H1_cam (Ad d) = (H1_cam Ad) d)
template <typename SA>
__device__ __forceinline__ void step_to_camera(const SA& S, double* d) {
  if constexpr (std::is_same_v<SA, SensorArg>) {
    const double w0 = d[0], w1 = d[1], w2 = d[2], v0 = d[3], v1 = d[4], v2 = d[5];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      d[rr] = sensor_A(S, rr, 0) * w0 + sensor_A(S, rr, 1) * w1 + sensor_A(S, rr, 2) * w2;
      d[3 + rr] = (S.B[3 * rr] * w0 + S.B[3 * rr + 1] * w1 + S.B[3 * rr + 2] * w2) +
                  (sensor_A(S, rr, 0) * v0 + sensor_A(S, rr, 1) * v1 + sensor_A(S, rr, 2) * v2);
    }
  }
}

// IRLS (Block reweighting): scale a factor's whitened residual and Jacobian rows by sqrt(w), w from its own residual
template <int LOSS, bool WITH_H1, bool WITH_H2>
__device__ __forceinline__ void robust_reweight(double k, double* r, double* H1, double* H2) {
  double w, rho;
  robust_weight<LOSS>(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], k, w, rho);
  const double s = sqrt(w);
#pragma unroll
  for (int q = 0; q < 3; ++q) r[q] *= s;
  if (WITH_H1)
#pragma unroll
    for (int q = 0; q < 18; ++q) H1[q] *= s;
  if (WITH_H2)
#pragma unroll
    for (int q = 0; q < 9; ++q) H2[q] *= s;
}

// ---------------------------------------------------------------------------------------------
// linearisation (LOSS = VUS_LOSS_*: the Gaussian instance is the plain statement, a robust one reweights every factor
// before the products; loss_k = the mEstimator's parameter, unused by the Gaussian instance.  SENSOR: the camera sits at
// X o S and H1 is taken to the body tangent before W = H1^T H2)
template <int LOSS, bool SENSOR = false, bool MIXED = false>
__global__ __launch_bounds__(256) void lin_points_kernel(vus_ba_problem P, const double* __restrict__ poses,
                                                         const double* __restrict__ points,
                                                         double* __restrict__ W, double* __restrict__ V,
                                                         double* __restrict__ gl, double* __restrict__ err_part,
                                                         double loss_k, sensor_arg_t<SENSOR> S, mono_arg_t<MIXED> M) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= P.n_points) return;
  const Calib K = load_calib(P.K, P.inv_sigma);
  const int a0 = P.point_ptr[j], a1 = P.point_ptr[j + 1];
  const double p[3] = {points[3 * j], points[3 * j + 1], points[3 * j + 2]};
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, e = 0;
  for (int a = a0 + lane; a < a1; a += 64) {
    double T[12], r[3], H1[18], H2[9];
    load_camera(poses + 12 * (size_t)P.obs_pose[a], S, T);
    obs_factor<true, true>(P, K, M, a, T, p, r, H1, H2);
    if (LOSS != VUS_LOSS_GAUSSIAN) robust_reweight<LOSS, true, true>(loss_k, r, H1, H2);
    h1_to_body(S, H1);
    e += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);      // robust: 0.5 w d^2, the linear error at delta = 0
    double* Wa = W + 18 * (size_t)a;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c) Wa[3 * rr + c] = H1[rr] * H2[c] + H1[6 + rr] * H2[3 + c] + H1[12 + rr] * H2[6 + c];
    int u = 0;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = rr; c < 3; ++c, ++u) v[u] += H2[rr] * H2[c] + H2[3 + rr] * H2[3 + c] + H2[6 + rr] * H2[6 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] += H2[c] * r[0] + H2[3 + c] * r[1] + H2[6 + c] * r[2];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = wave_sum(g[k]);
  e = wave_sum(e);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) V[6 * (size_t)j + k] = v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) gl[3 * (size_t)j + k] = g[k];
    err_part[j] = e;
  }
}

// SENSOR: Ad(S^-1) is the same for all of a pose's factors, so the sums are taken in the CAMERA tangent as without an
// extrinsic and the epilogue applies Hpp = Ad^T (.) Ad, gp = Ad^T (.) once per workgroup
template <int LOSS, bool SENSOR = false, bool MIXED = false>
__global__ __launch_bounds__(256) void lin_poses_kernel(vus_ba_problem P, const double* __restrict__ poses,
                                                        const double* __restrict__ points,
                                                        double* __restrict__ Hpp, double* __restrict__ gp,
                                                        double loss_k, sensor_arg_t<SENSOR> S, mono_arg_t<MIXED> M) {
  __shared__ double s_part[4][27];
  const int i = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Calib K = load_calib(P.K, P.inv_sigma);
  double T[12];
  load_camera(poses + 12 * (size_t)i, S, T);
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0;
  const int s0 = P.pose_ptr[i], s1 = P.pose_ptr[i + 1];
  for (int s = s0 + (int)threadIdx.x; s < s1; s += 256) {
    const int a = P.pobs_lidx[s];
    const int j = P.obs_point[a];
    const double p[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
    double r[3], H1[18];
    obs_factor<true, false>(P, K, M, a, T, p, r, H1, nullptr);
    if (LOSS != VUS_LOSS_GAUSSIAN) robust_reweight<LOSS, true, false>(loss_k, r, H1, nullptr);
    int u = 0;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
      for (int c = rr; c < 6; ++c, ++u) acc[u] += H1[rr] * H1[c] + H1[6 + rr] * H1[6 + c] + H1[12 + rr] * H1[12 + c];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) acc[21 + rr] += H1[rr] * r[0] + H1[6 + rr] * r[1] + H1[12 + rr] * r[2];
  }
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 27; ++k) s_part[wave][k] = acc[k];
  __syncthreads();
  double sum = 0;
  if (threadIdx.x < 36) {
    const int rr = threadIdx.x / 6, c = threadIdx.x % 6;
    const int lo = rr < c ? rr : c, hi = rr < c ? c : rr;
    const int u = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);  // index in the row-wise upper triangle
    sum = ((s_part[0][u] + s_part[1][u]) + s_part[2][u]) + s_part[3][u];
    if (!SENSOR) Hpp[36 * (size_t)i + threadIdx.x] = sum;
  } else if (threadIdx.x < 42) {
    const int u = 21 + threadIdx.x - 36;
    sum = ((s_part[0][u] + s_part[1][u]) + s_part[2][u]) + s_part[3][u];
    if (!SENSOR) gp[6 * (size_t)i + threadIdx.x - 36] = sum;
  }
  if constexpr (SENSOR) {
    // the camera-tangent sums expanded to the full 6 x 6 and the 6-vector, Ad(S^-1) beside them, then the congruence
    __shared__ double s_hg[42], s_ad[36];
    if (threadIdx.x < 42) s_hg[threadIdx.x] = sum;
    if (threadIdx.x == 64) {      // lane 0 of a wave with nothing else to do here: constant indices into the arguments
#pragma unroll
      for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s_ad[6 * rr + c] = sensor_A(S, rr, c);
          s_ad[6 * rr + 3 + c] = 0.0;
          s_ad[6 * (rr + 3) + c] = S.B[3 * rr + c];
          s_ad[6 * (rr + 3) + 3 + c] = sensor_A(S, rr, c);
        }
    }
    __syncthreads();
    if (threadIdx.x < 36) {
      const int rr = threadIdx.x / 6, c = threadIdx.x % 6;
      double out = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double mk = 0;      // (H Ad)[k][c]
#pragma unroll
        for (int l = 0; l < 6; ++l) mk += s_hg[6 * k + l] * s_ad[6 * l + c];
        out += s_ad[6 * k + rr] * mk;
      }
      Hpp[36 * (size_t)i + threadIdx.x] = out;
    } else if (threadIdx.x < 42) {
      const int rr = threadIdx.x - 36;
      double out = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) out += s_ad[6 * k + rr] * s_hg[36 + k];
      gp[6 * (size_t)i + rr] = out;
    }
  }
}

// PriorFactorPose3 (gtsam PriorFactor::evaluateError: e = -Local(x, prior), H = I), one lane, in order.
// mode 0: add information/gradient into Hpp/gp and write the error to err_out[0]
// mode 1: error only;  mode 2: linearised error 0.5|r + w dp|^2 at OLD poses to err_out[0]
__global__ void priors_kernel(vus_ba_problem P, const double* __restrict__ poses, const double* __restrict__ dp,
                              double* __restrict__ Hpp, double* __restrict__ gp, double* __restrict__ err_out,
                              int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double e = 0;
  for (int q = 0; q < P.n_priors; ++q) {
    const int i = P.prior_pose[q];
    double xi[6];
    pose_local(poses + 12 * (size_t)i, P.prior_T + 12 * (size_t)q, xi);
    for (int k = 0; k < 6; ++k) {
      const double w = P.prior_w[6 * (size_t)q + k];
      double r = -xi[k] * w;
      if (mode == 0) {
        Hpp[36 * (size_t)i + 7 * k] += w * w;
        gp[6 * (size_t)i + k] += w * r;
      }
      if (mode == 2) r += w * dp[6 * (size_t)pose_stride(P) * i + k];
      e += 0.5 * r * r;
    }
  }
  err_out[0] = e;
}

// ---------------------------------------------------------------------------------------------
// damped landmark elimination
__global__ void vinv_kernel(int n_points, double lambda, const double* __restrict__ V, double* __restrict__ Vinv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_points) return;
  const double a = V[6 * (size_t)j] + lambda, b = V[6 * (size_t)j + 1], c = V[6 * (size_t)j + 2];
  const double d = V[6 * (size_t)j + 3] + lambda, e = V[6 * (size_t)j + 4], f = V[6 * (size_t)j + 5] + lambda;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double id = 1.0 / (a * c00 + b * c01 + c * c02);
  double* o = Vinv + 6 * (size_t)j;
  o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
  o[3] = (a * f - c * c) * id; o[4] = (b * c - a * e) * id; o[5] = (a * d - b * b) * id;
}

__global__ void ymul_kernel(vus_ba_problem P, const double* __restrict__ W, const double* __restrict__ Vinv,
                            double* __restrict__ Y) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;      // L-order row
  if (s >= P.n_obs) return;
  const int j = P.obs_point[s];
  double vi[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) vi[k] = Vinv[6 * (size_t)j + k];
  const double* Ws = W + 18 * (size_t)s;
  double* Ys = Y + 18 * (size_t)s;
#pragma unroll
  for (int rr = 0; rr < 6; ++rr) {
    const double w0 = Ws[3 * rr], w1 = Ws[3 * rr + 1], w2 = Ws[3 * rr + 2];
    Ys[3 * rr + 0] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
    Ys[3 * rr + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
    Ys[3 * rr + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
  }
}

// ---------------------------------------------------------------------------------------------
// The landmark elimination on the matrix cores: S(I,K) = init - sum_j A_j B_j^T per 8 x 8-pose tile pair (include/vus.h,
// vus_ba_tiles), the sum over the landmarks being the K dimension of a GEMM.  A workgroup of four waves owns one unit at
// a time (persistent, units handed out largest first through a global counter).  A wave takes the chunks c = wave,
// wave + 4, ... of the unit's landmark list, ST_CH landmarks each: it stages A = [W_ij Vinv_j] and B = [W_kj] of the chunk
// K-MAJOR into its own LDS panels (panel[k][row], row = 6 * pose + component: an MFMA operand fetch is 16 consecutive
// doubles per k), zero rows where a pose does not see the landmark, and runs the 3 x 3 output tiles of 16 x 16 over the
// chunk's K = 3 ST_CH columns.  Software-pipelined inside the wave: while the matrix cores work on chunk c, the W rows of
// chunk c + 1 and the entry of chunk c + 2 are in flight (two dependent loads deep: entry -> rows) -- with 77 KB of LDS
// per workgroup in panels only two waves per SIMD are resident and nothing else would hide a memory round trip.  No
// workgroup barrier inside a unit: the panels are wave-private, LDS operations of one wave complete in order.  The four
// partial tiles meet in LDS at the end (fixed order: no result depends on scheduling, bit-identical from run to run) and
// leave as 16-byte vectors in the band's address order.  W is in L-order: a landmark's rows of a tile are consecutive.
//
// Measured at configs[2] (profiles/r04_summary.md; 2000 keyframes, 50,238 landmarks, 2.0 M factors, 1.82 M entries): the
// per-pair vector kernel of rounds 1-3 1.36 ms (2.6 ms once a pose has more than 1000 observations) + 0.11 ms for the
// right-hand side; this kernel 0.65 ms including it.  Steps on the way (same box A/B, tools/schur_ab.py): W gathered
// through obs_ppos 1.66 -> W in L-order 1.23 -> pipelined 0.86 -> one entry and Vinv per lane in registers instead of LDS
// tables, operands of the next K step requested before the products of this one, conflict-free panel writes 0.77 ->
// right-hand side fused 0.69.  One queue of units per XCD in natural order (neighbouring tile rows together on one L2)
// raised the L2 hit rate from 16 % to 42 % and was SLOWER (0.79): the kernel is not memory-bound -- with every row read
// from a cache-resident 4096-row window it takes 0.85 instead of 0.89 ms -- but a unit is up to 1638 entries = 40 % of the
// kernel's duration for its workgroup, so the largest-first order matters more than locality.
constexpr int ST_CH = 8;                       // landmarks per chunk
constexpr int ST_KC = 3 * ST_CH;               // K columns per chunk: 6 steps of v_mfma_f64_16x16x4
constexpr int ST_LD = 50;                      // panel stride in doubles (48 rows + 2)
constexpr int ST_PANEL = ST_KC * ST_LD;
constexpr int ST_WAVES = 4;
constexpr int ST_WAVE_DOUBLES = 2 * ST_PANEL + ST_KC + 8;                 // the two panels, gl by K row (+ padding to 16 bytes)
static_assert(2 * ST_PANEL >= 48 * 48, "a wave's panels also hold its partial 48 x 48 tile");
static_assert(ST_KC % 4 == 0, "whole MFMA K steps");

__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__global__ __launch_bounds__(64 * ST_WAVES, 2) void schur_tiles_kernel(vus_ba_tiles T, int n_poses, int ps, int band_nodes,
                                                                        double lambda, const double* __restrict__ W,
                                                                        const double* __restrict__ Vinv,
                                                                        const double* __restrict__ Hpp,
                                                                        const double* __restrict__ gl, const double* __restrict__ gp,
                                                                        double* __restrict__ Sband, double* __restrict__ gs,
                                                                        int* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) double st_smem[];
  __shared__ int s_unit;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  double* __restrict__ PA = st_smem + wave * ST_WAVE_DOUBLES;
  double* __restrict__ PB = PA + ST_PANEL;
  double* __restrict__ gtab = PB + ST_PANEL;      // [ST_KC]: gl of the chunk's landmarks by K row (tile pairs (I, I) only)
  const int4* __restrict__ entries = reinterpret_cast<const int4*>(T.entries);
  const int dt1 = T.n_units / T.n_tiles;
  const int arow = lane & 15, kq = lane >> 4;
  // lane = 8 * landmark of the chunk + sub: the lane's six tasks per side are rows qr = 8 rnd + sub of ITS landmark, so one
  // entry and one Vinv per lane and chunk, straight from memory into registers (no LDS tables, no dependent LDS reads in
  // the staging pass); the eight lanes of a landmark read 192 contiguous bytes per round.
  const int tl = lane >> 3, sub = lane & 7, krow = (tl >> 1) + 4 * (tl & 1);
  int tq[6], tr[6];
#pragma unroll
  for (int rnd = 0; rnd < 6; ++rnd) {
    tq[rnd] = (8 * rnd + sub) / 6;
    tr[rnd] = (8 * rnd + sub) - 6 * tq[rnd];
  }
  while (true) {
    __syncthreads();                 // the previous unit's partial tiles have been consumed, s_unit has been read
    if (tid == 0) s_unit = atomicAdd(counter, 1);
    __syncthreads();
    const int ui = s_unit;
    if (ui >= T.n_units) break;
    const int u = T.order[ui];
    const int I = u / dt1, d = u - I * dt1, K = I - d;
    if (K < 0) continue;
    const bool diag = d == 0;
    const int e0 = T.unit_ptr[u], e1 = T.unit_ptr[u + 1];
    const int n_chunks = (e1 - e0 + ST_CH - 1) / ST_CH;
    double4_t acc[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[t][q] = double4_t{0.0, 0.0, 0.0, 0.0};
    // pipeline registers
    int4 en;               // the lane's entry of the chunk whose rows are requested next
    double wa[6][3], wb[6][3], vi[6], gv = 0.0;
    unsigned pres = 0;     // bit rnd / 6 + rnd: the task's pose sees the landmark (side A / B)
    // (nothing may touch `en` between its load and load_rows: a use would make the compiler wait for it at once, and with
    // it -- the memory counter is in-order -- for every row load issued just before: the whole prefetch would be lost)
    auto load_entries = [&](int c) {
      const int e = e0 + ST_CH * c + tl;
      en = entries[e < e1 ? e : e0];
    };
    auto load_rows = [&](int c) {     // from en (arrived): the W rows of chunk c and the landmark's Vinv
      pres = 0;
      const bool valid = e0 + ST_CH * c + tl < e1;
      const int ma = valid ? en.w & 0xFF : 0, mb = valid ? (en.w >> 8) & 0xFF : 0;
#pragma unroll
      for (int rnd = 0; rnd < 6; ++rnd) {
        const int bit = 1 << tq[rnd], below = bit - 1;
        const bool pa = ma & bit, pb = mb & bit;
        pres |= (pa ? 1u : 0u) << rnd | (pb ? 1u : 0u) << (6 + rnd);
        const double* ra = W + 18 * (size_t)(en.x + (pa ? __popc(ma & below) : 0)) + 3 * tr[rnd];
        const double* rb = W + 18 * (size_t)(en.y + (pb ? __popc(mb & below) : 0)) + 3 * tr[rnd];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          wa[rnd][k] = ra[k];
          wb[rnd][k] = rb[k];
        }
      }
      const double* vsrc = Vinv + 6 * (size_t)en.z;
#pragma unroll
      for (int k = 0; k < 6; ++k) vi[k] = vsrc[k];
      if (diag) gv = valid && sub < 3 ? gl[3 * (size_t)en.z + sub] : 0.0;      // the reduced right-hand side rides along
    };
    if (wave < n_chunks) {
      load_entries(wave);
      load_rows(wave);
      if (wave + ST_WAVES < n_chunks) load_entries(wave + ST_WAVES);
    }
    for (int c = wave; c < n_chunks; c += ST_WAVES) {
      // chunk c: rows (arrived during the previous chunk's products) -> panels
      if (diag && sub < 3) gtab[8 * sub + krow] = gv;
#pragma unroll
      for (int rnd = 0; rnd < 6; ++rnd) {
        const bool pa = (pres >> rnd) & 1, pb = (pres >> (6 + rnd)) & 1;
        const double a0 = pa ? wa[rnd][0] : 0.0, a1 = pa ? wa[rnd][1] : 0.0, a2 = pa ? wa[rnd][2] : 0.0;
        // K row of (landmark tl, column c) = 8 c + krow: which K index holds what is free as long as both panels agree.
        // ds_write_b64 is served in groups of 16 consecutive lanes = two landmarks: with a stride of 50 doubles their
        // rows must lie 4 apart to fall on disjoint banks (4 * 100 dwords = 16 mod 32)
        double* da = PA + krow * ST_LD + 8 * rnd + sub;
        da[0] = a0 * vi[0] + a1 * vi[1] + a2 * vi[2];
        da[8 * ST_LD] = a0 * vi[1] + a1 * vi[3] + a2 * vi[4];
        da[16 * ST_LD] = a0 * vi[2] + a1 * vi[4] + a2 * vi[5];
        double* db = PB + krow * ST_LD + 8 * rnd + sub;
        db[0] = pb ? wb[rnd][0] : 0.0;
        db[8 * ST_LD] = pb ? wb[rnd][1] : 0.0;
        db[16 * ST_LD] = pb ? wb[rnd][2] : 0.0;
      }
      // chunk c + 1: its entries have arrived -> request its rows; chunk c + 2: request its entries
      if (c + ST_WAVES < n_chunks) {
        load_rows(c + ST_WAVES);
        if (c + 2 * ST_WAVES < n_chunks) load_entries(c + 2 * ST_WAVES);
      }
      wave_lds_fence();
      {
        double a[2][3], b[2][3];     // the operands of step s2 + 1 are requested before the products of step s2 are issued
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          a[0][t] = PA[kq * ST_LD + 16 * t + arow];
          b[0][t] = PB[kq * ST_LD + 16 * t + arow];
        }
#pragma unroll
        for (int s2 = 0; s2 < ST_KC / 4; ++s2) {
          const int cur = s2 & 1, nxt = cur ^ 1;
          if (s2 + 1 < ST_KC / 4) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
              a[nxt][t] = PA[(4 * (s2 + 1) + kq) * ST_LD + 16 * t + arow];
              b[nxt][t] = PB[(4 * (s2 + 1) + kq) * ST_LD + 16 * t + arow];
            }
          }
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int q = 0; q <= t; ++q) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][t], b[cur][q], acc[t][q], 0, 0, 0);
          // Of the tile pair (I, I) the 16 x 16 tiles above the diagonal are not stored: their accumulators take
          // Y gl instead -- a B operand whose column 0 is gl along K and whose other columns are zero -- so column 0 of
          // the three tiles is sum_j Y_ij Vinv_j... = what gs subtracts, rows 0-15, 16-31, 32-47
          const double bg = diag && arow == 0 ? gtab[4 * s2 + kq] : 0.0;
          acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][0], diag ? bg : b[cur][1], acc[0][1], 0, 0, 0);
          acc[0][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(diag ? a[cur][1] : a[cur][0], diag ? bg : b[cur][2], acc[0][2], 0, 0, 0);
          acc[1][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(diag ? a[cur][2] : a[cur][1], diag ? bg : b[cur][2], acc[1][2], 0, 0, 0);
        }
      }
      wave_lds_fence();
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) PA[(16 * t + kq + 4 * r) * 48 + 16 * q + arow] = acc[t][q][r];
    __syncthreads();
    for (int v = tid; v < 8 * 144; v += 64 * ST_WAVES) {
      const int ii = v / 144, w = v - 144 * ii, o = w / 18, e = 2 * (w - 18 * o), kk = 7 - o;
      const int i = 8 * I + ii, k = 8 * K + kk;
      if (i >= n_poses || k > i || ps * (i - k) > band_nodes) continue;
      const int rr = e / 6, cc = e - 6 * rr;
      // a diagonal block is written whole: its elements above the diagonal come from their mirror images (of the tile pair
      // (I, I) only the 16 x 16 tiles on and below the diagonal are computed)
      const bool dblk = i == k;
      const int at0 = dblk && cc > rr ? (6 * ii + cc) * 48 + 6 * kk + rr : (6 * ii + rr) * 48 + 6 * kk + cc;
      const int at1 = dblk && cc + 1 > rr ? (6 * ii + cc + 1) * 48 + 6 * kk + rr : (6 * ii + rr) * 48 + 6 * kk + cc + 1;
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int wv = 0; wv < ST_WAVES; ++wv) {
        s0 += st_smem[wv * ST_WAVE_DOUBLES + at0];
        s1 += st_smem[wv * ST_WAVE_DOUBLES + at1];
      }
      d2a_t out = d2a_t{-s0, -s1};
      if (i == k) {
        out.x += Hpp[36 * (size_t)i + e] + (rr == cc ? lambda : 0.0);
        out.y += Hpp[36 * (size_t)i + e + 1] + (rr == cc + 1 ? lambda : 0.0);
      }
      *reinterpret_cast<d2a_t*>(Sband + 36 * ((size_t)(ps * i) * (band_nodes + 1) + (size_t)ps * (i - k)) + e) = out;
    }
    if (diag && tid < 48 && 8 * I + tid / 6 < n_poses) {      // gs rows of the tile's poses: column 0 of the three spare tiles
      const int m = tid, t = m >> 4, mm = m & 15;
      const int at = t == 0 ? mm * 48 + 16 : (t == 1 ? mm * 48 + 32 : (16 + mm) * 48 + 32);
      double sg = 0.0;
#pragma unroll
      for (int wv = 0; wv < ST_WAVES; ++wv) sg += st_smem[wv * ST_WAVE_DOUBLES + at];
      const int i = 8 * I + m / 6;
      gs[6 * (size_t)(ps * i) + (m - 6 * (m / 6))] = gp[6 * (size_t)i + (m - 6 * (m / 6))] - sg;
    }
  }
}

// slots (i, s) with s > i of the first `band` rows lie left of pose 0: never read, kept at zero (one workgroup per row)
__global__ void band_head_zero_kernel(double* __restrict__ Sband, int n_poses, int band) {
  const int i = blockIdx.x;
  double* row = Sband + 36 * ((size_t)i * (band + 1) + (i + 1));
  for (int t = threadIdx.x; t < 36 * (band - i); t += blockDim.x) row[t] = 0.0;
}

__global__ void add_diag_kernel(double* __restrict__ Sband, int n_poses, int band, double value) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 6 * n_poses) Sband[36 * (size_t)(t / 6) * (band + 1) + 7 * (t % 6)] += value;
}

// ---------------------------------------------------------------------------------------------
// back-substitution, retraction, error evaluation
__global__ __launch_bounds__(256) void backsub_kernel(vus_ba_problem P, const double* __restrict__ W,
                                                      const double* __restrict__ Vinv,
                                                      const double* __restrict__ gl, const double* __restrict__ dp,
                                                      double* __restrict__ dl) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= P.n_points) return;
  double t[3] = {0, 0, 0};
  for (int a = P.point_ptr[j] + lane; a < P.point_ptr[j + 1]; a += 64) {
    const double* Wa = W + 18 * (size_t)a;
    const double* d = dp + 6 * (size_t)pose_stride(P) * P.obs_pose[a];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
      const double dr = d[rr];
      t[0] += Wa[3 * rr] * dr;
      t[1] += Wa[3 * rr + 1] * dr;
      t[2] += Wa[3 * rr + 2] * dr;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = wave_sum(t[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] += gl[3 * (size_t)j + c];
    const double* vi = Vinv + 6 * (size_t)j;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dl[3 * (size_t)j + c] = -(sym3(vi, c, 0) * t[0] + sym3(vi, c, 1) * t[1] + sym3(vi, c, 2) * t[2]);
  }
}

__global__ void retract_kernel(int n_poses, int n_points, int ps, const double* __restrict__ poses,
                               const double* __restrict__ points, const double* __restrict__ dp,
                               const double* __restrict__ dl, double* __restrict__ new_poses,
                               double* __restrict__ new_points) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_poses) {
    double T[12], xi[6], out[12];
    load12(poses + 12 * (size_t)t, T);
#pragma unroll
    for (int k = 0; k < 6; ++k) xi[k] = dp[6 * (size_t)ps * t + k];
    pose_retract(T, xi, out);
#pragma unroll
    for (int k = 0; k < 12; ++k) new_poses[12 * (size_t)t + k] = out[k];
  }
  for (int k = t; k < 3 * n_points; k += gridDim.x * blockDim.x) new_points[k] = points[k] + dl[k];
}

// per point: part_lin[j] = 0.5 sum |r + H1 dp + H2 dl|^2 at the old values,
//            part_new[j] = 0.5 sum |r|^2 at the new values
// robust LOSS: r, H1, H2 at the old values reweighted by sqrt(w(old)) (the linearisation point), part_new = sum rho
// SENSOR: both the old and the new poses are composed with S; dp is a body-tangent step, taken to the camera tangent
template <bool WITH_LIN, int LOSS = VUS_LOSS_GAUSSIAN, bool SENSOR = false, bool MIXED = false>
__global__ __launch_bounds__(256) void eval_points_kernel(vus_ba_problem P, const double* __restrict__ poses,
                                                          const double* __restrict__ points,
                                                          const double* __restrict__ dp, const double* __restrict__ dl,
                                                          const double* __restrict__ new_poses,
                                                          const double* __restrict__ new_points,
                                                          double* __restrict__ part_lin, double* __restrict__ part_new,
                                                          double loss_k, sensor_arg_t<SENSOR> S, mono_arg_t<MIXED> M) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= P.n_points) return;
  const Calib K = load_calib(P.K, P.inv_sigma);
  const double pn[3] = {new_points[3 * (size_t)j], new_points[3 * (size_t)j + 1], new_points[3 * (size_t)j + 2]};
  double po[3] = {0, 0, 0}, d_l[3] = {0, 0, 0};
  if (WITH_LIN) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      po[c] = points[3 * (size_t)j + c];
      d_l[c] = dl[3 * (size_t)j + c];
    }
  }
  double e_lin = 0, e_new = 0;
  for (int a = P.point_ptr[j] + lane; a < P.point_ptr[j + 1]; a += 64) {
    const int i = P.obs_pose[a];
    double T[12], r[3];
    load_camera(new_poses + 12 * (size_t)i, S, T);
    obs_factor<false, false>(P, K, M, a, T, pn, r, nullptr, nullptr);
    if (LOSS == VUS_LOSS_GAUSSIAN) {
      e_new += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    } else {
      double w, rho;
      robust_weight<LOSS>(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], loss_k, w, rho);
      e_new += rho;
    }
    if (WITH_LIN) {
      double H1[18], H2[9];
      load_camera(poses + 12 * (size_t)i, S, T);
      obs_factor<true, true>(P, K, M, a, T, po, r, H1, H2);
      if (LOSS != VUS_LOSS_GAUSSIAN) robust_reweight<LOSS, true, true>(loss_k, r, H1, H2);
      double d[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) d[c] = dp[6 * (size_t)pose_stride(P) * i + c];
      step_to_camera(S, d);
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) {
        double t = r[rr];
#pragma unroll
        for (int c = 0; c < 6; ++c) t += H1[6 * rr + c] * d[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) t += H2[3 * rr + c] * d_l[c];
        e_lin += 0.5 * t * t;
      }
    }
  }
  e_new = wave_sum(e_new);
  if (WITH_LIN) e_lin = wave_sum(e_lin);
  if (lane == 0) {
    part_new[j] = e_new;
    if (WITH_LIN) part_lin[j] = e_lin;
  }
}

int check_problem(const vus_ba_problem* P) {
  VUS_REQUIRE(P != nullptr, "problem is null");
  VUS_REQUIRE(P->n_poses >= 1 && P->n_points >= 0 && P->n_obs >= 0 && P->n_priors >= 0,
              "bad sizes: poses=%d points=%d obs=%d priors=%d", P->n_poses, P->n_points, P->n_obs, P->n_priors);
  VUS_REQUIRE(P->K != nullptr, "K is null");
  VUS_REQUIRE(P->inv_sigma > 0.0, "inv_sigma=%g", P->inv_sigma);
  // pose_ptr has n_poses + 1 entries and the per-pose kernels read it even for a graph without a stereo factor
  VUS_REQUIRE(P->pose_ptr != nullptr, "pose_ptr is null");
  if (P->n_points > 0) VUS_REQUIRE(P->point_ptr != nullptr, "point_ptr is null");
  if (P->n_obs > 0)
    VUS_REQUIRE(P->meas && P->obs_pose && P->obs_point && P->point_ptr && P->obs_ppos && P->pobs_lidx,
                "observation arrays are null");
  if (P->n_priors > 0) VUS_REQUIRE(P->prior_pose && P->prior_T && P->prior_w, "prior arrays are null");
  return VUS_OK;
}

// w [n_obs] (L-order) of every stereo observation at (poses, points), thread / observation
template <int LOSS, bool SENSOR = false, bool MIXED = false>
__global__ __launch_bounds__(256) void stereo_weights_kernel(vus_ba_problem P, const double* __restrict__ poses,
                                                             const double* __restrict__ points, double* __restrict__ w_out,
                                                             double loss_k, sensor_arg_t<SENSOR> S, mono_arg_t<MIXED> M) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= P.n_obs) return;
  const Calib K = load_calib(P.K, P.inv_sigma);
  const int j = P.obs_point[a];
  const double p[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
  double T[12], r[3], w, rho;
  load_camera(poses + 12 * (size_t)P.obs_pose[a], S, T);
  obs_factor<false, false>(P, K, M, a, T, p, r, nullptr, nullptr);
  robust_weight<LOSS>(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], loss_k, w, rho);
  w_out[a] = w;
}

int check_loss(const vus_ba_loss* L) {
  VUS_REQUIRE(L != nullptr, "loss is null");
  VUS_REQUIRE(L->kind >= VUS_LOSS_GAUSSIAN && L->kind <= VUS_LOSS_WELSCH, "unknown loss kind %d", L->kind);
  VUS_REQUIRE(L->kind == VUS_LOSS_GAUSSIAN || (L->k > 0.0 && L->k <= 1.7976931348623157e308),
              "loss parameter k=%g must be finite and > 0", L->k);
  return VUS_OK;
}

// vus_ba_sensor -> the kernels' SensorArg, validated on the host (include/vus_sensor.h)
int make_sensor(const vus_ba_sensor* s, SensorArg& out) {
  VUS_REQUIRE(s != nullptr, "sensor is null");
  for (int k = 0; k < 12; ++k) VUS_REQUIRE(std::isfinite(s->T[k]), "sensor: T[%d]=%g is not finite", k, s->T[k]);
  const double* R = s->T;
  const double* t = s->T + 9;
  double worst = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double g = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - (a == b ? 1.0 : 0.0);
      worst = std::fmax(worst, std::fabs(g));
    }
  VUS_REQUIRE(worst <= 1e-9, "sensor: the rotation is not orthonormal (max |R^T R - I| = %g)", worst);
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  VUS_REQUIRE(det > 0.0, "sensor: the rotation is a reflection (det = %g)", det);
  for (int k = 0; k < 12; ++k) out.T[k] = s->T[k];
  const double tx[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};      // [ts]x
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      out.B[3 * a + b] = -(R[a] * tx[b] + R[3 + a] * tx[3 + b] + R[6 + a] * tx[6 + b]);
    }
  return VUS_OK;
}

// vus_ba_mono -> the kernels' MonoArg, validated on the host (include/vus_mono.h)
int make_mono(const vus_ba_problem* P, const vus_ba_mono* m, MonoArg& out) {
  VUS_REQUIRE(m != nullptr, "mono is null");
  for (int k = 0; k < 5; ++k) VUS_REQUIRE(std::isfinite(m->K[k]), "mono: K[%d]=%g is not finite", k, m->K[k]);
  VUS_REQUIRE(m->K[0] > 0.0 && m->K[1] > 0.0, "mono: fx=%g fy=%g must be > 0", m->K[0], m->K[1]);
  VUS_REQUIRE(std::isfinite(m->inv_sigma) && m->inv_sigma > 0.0, "mono: inv_sigma=%g must be finite and > 0", m->inv_sigma);
  VUS_REQUIRE(m->is_mono != nullptr || !P || P->n_obs <= 0, "mono: is_mono is null");
  out = MonoArg{m->is_mono, m->K[0], m->K[1], m->K[2], m->K[3], m->K[4], m->inv_sigma};
  return VUS_OK;
}

// f(sensor argument, mono argument) with the kernels' argument types of the (SENSOR, MIXED) instance a call takes
template <typename F>
void with_variant(const SensorArg* S, const MonoArg* M, F f) {
  if (S && M) f(*S, *M);
  else if (S) f(*S, NoMono{});
  else if (M) f(NoSensor{}, *M);
  else f(NoSensor{}, NoMono{});
}
template <typename SA>
constexpr bool is_sensor_v = std::is_same_v<SA, SensorArg>;
template <typename MA>
constexpr bool is_mono_v = std::is_same_v<MA, MonoArg>;

// one instance of F<LOSS> per kind, chosen at run time (the loss was validated by check_loss)
template <template <int> class F, typename... A>
int dispatch_loss(const vus_ba_loss* L, A... args) {
  switch (L->kind) {
    case VUS_LOSS_HUBER: return F<VUS_LOSS_HUBER>::run(L->k, args...);
    case VUS_LOSS_CAUCHY: return F<VUS_LOSS_CAUCHY>::run(L->k, args...);
    case VUS_LOSS_TUKEY: return F<VUS_LOSS_TUKEY>::run(L->k, args...);
    case VUS_LOSS_GEMAN_MCCLURE: return F<VUS_LOSS_GEMAN_MCCLURE>::run(L->k, args...);
    case VUS_LOSS_WELSCH: return F<VUS_LOSS_WELSCH>::run(L->k, args...);
    default: return F<VUS_LOSS_GAUSSIAN>::run(0.0, args...);
  }
}

template <int LOSS>
struct ErrorOp {
  static int run(double k, const vus_ba_problem* P, const double* poses, const double* points, double* err,
                 double* work, void* stream, const SensorArg* S, const MonoArg* M) {
    if (int rc = check_problem(P)) return rc;
    VUS_REQUIRE(poses && (points || !P->n_points) && err && work, "null buffer");
    hipStream_t st = vus::as_stream(stream);
    const int nL = P->n_points;
    if (nL > 0)
      with_variant(S, M, [&](auto s, auto m) {
        eval_points_kernel<false, LOSS, is_sensor_v<decltype(s)>, is_mono_v<decltype(m)>><<<cdiv(nL, 4), 256, 0, st>>>(
            *P, nullptr, nullptr, nullptr, nullptr, poses, points, nullptr, work, k, s, m);
      });
    priors_kernel<<<1, 64, 0, st>>>(*P, poses, nullptr, nullptr, nullptr, work + nL, 1);
    vus::reduce_partials(work, nL + 1, err, st);
    VUS_CHECK_LAUNCH("ba_error");
    return VUS_OK;
  }
};

template <int LOSS>
struct LinearizeOp {
  static int run(double k, const vus_ba_problem* P, const double* poses, const double* points, double* W, double* V,
                 double* gl, double* Hpp, double* gp, double* err, double* work, void* stream, const SensorArg* S,
                 const MonoArg* M) {
    if (int rc = check_problem(P)) return rc;
    // a graph without landmarks (priors only) has empty per-landmark / per-observation arrays: those may be null
    VUS_REQUIRE(poses && Hpp && gp && err && work, "null buffer");
    VUS_REQUIRE((points && V && gl) || !P->n_points, "null landmark buffer");
    VUS_REQUIRE(W || !P->n_obs, "null observation buffer");
    hipStream_t st = vus::as_stream(stream);
    const int nL = P->n_points;
    with_variant(S, M, [&](auto s, auto m) {
      constexpr bool SE = is_sensor_v<decltype(s)>, MI = is_mono_v<decltype(m)>;
      if (nL > 0) lin_points_kernel<LOSS, SE, MI><<<cdiv(nL, 4), 256, 0, st>>>(*P, poses, points, W, V, gl, work, k, s, m);
      lin_poses_kernel<LOSS, SE, MI><<<P->n_poses, 256, 0, st>>>(*P, poses, points, Hpp, gp, k, s, m);
    });
    priors_kernel<<<1, 64, 0, st>>>(*P, poses, nullptr, Hpp, gp, work + nL, 0);
    vus::reduce_partials(work, nL + 1, err, st);
    VUS_CHECK_LAUNCH("ba_linearize");
    return VUS_OK;
  }
};

template <int LOSS>
struct EvalStepOp {
  static int run(double k, const vus_ba_problem* P, const double* poses, const double* points, const double* dp,
                 const double* dl, double* new_poses, double* new_points, double* out, double* work, void* stream,
                 const SensorArg* S, const MonoArg* M) {
    if (int rc = check_problem(P)) return rc;
    VUS_REQUIRE(poses && dp && new_poses && out && work, "null buffer");
    VUS_REQUIRE((points && dl && new_points) || !P->n_points, "null landmark buffer");
    hipStream_t st = vus::as_stream(stream);
    const int nP = P->n_poses, nL = P->n_points;
    retract_kernel<<<cdiv(nP > nL ? nP : (nL < 65536 ? nL : 65536), 256) + 1, 256, 0, st>>>(nP, nL, pose_stride(*P), poses, points,
                                                                                             dp, dl, new_poses, new_points);
    double* part_lin = work;
    double* part_new = work + (nL + 1);
    if (nL > 0)
      with_variant(S, M, [&](auto s, auto m) {
        eval_points_kernel<true, LOSS, is_sensor_v<decltype(s)>, is_mono_v<decltype(m)>><<<cdiv(nL, 4), 256, 0, st>>>(
            *P, poses, points, dp, dl, new_poses, new_points, part_lin, part_new, k, s, m);
      });
    priors_kernel<<<1, 64, 0, st>>>(*P, poses, dp, nullptr, nullptr, part_lin + nL, 2);
    priors_kernel<<<1, 64, 0, st>>>(*P, new_poses, nullptr, nullptr, nullptr, part_new + nL, 1);
    vus::reduce_partials(part_lin, nL + 1, out, st);
    vus::reduce_partials(part_new, nL + 1, out + 1, st);
    VUS_CHECK_LAUNCH("ba_eval_step");
    return VUS_OK;
  }
};

template <int LOSS>
struct WeightsOp {
  static int run(double k, const vus_ba_problem* P, const double* poses, const double* points, double* w, void* stream,
                 const SensorArg* S, const MonoArg* M) {
    if (int rc = check_problem(P)) return rc;
    VUS_REQUIRE(poses && ((points && w) || !P->n_obs), "null buffer");
    if (P->n_obs > 0)
      with_variant(S, M, [&](auto s, auto m) {
        stereo_weights_kernel<LOSS, is_sensor_v<decltype(s)>, is_mono_v<decltype(m)>>
            <<<cdiv(P->n_obs, 256), 256, 0, vus::as_stream(stream)>>>(*P, poses, points, w, k, s, m);
      });
    VUS_CHECK_LAUNCH("ba_stereo_weights");
    return VUS_OK;
  }
};

}  // namespace

extern "C" long long vus_ba_work_doubles(const vus_ba_problem* P) {
  if (!P) return 0;
  return 2ll * ((long long)P->n_points + 1) + 8;
}

extern "C" int vus_ba_error(const vus_ba_problem* P, const double* poses, const double* points, double* err,
                            double* work, void* stream) {
  return ErrorOp<VUS_LOSS_GAUSSIAN>::run(0.0, P, poses, points, err, work, stream, nullptr, nullptr);
}

extern "C" int vus_ba_error_robust(const vus_ba_problem* P, const double* poses, const double* points, double* err,
                                   double* work, void* stream, const vus_ba_loss* loss) {
  if (int rc = check_loss(loss)) return rc;
  return dispatch_loss<ErrorOp>(loss, P, poses, points, err, work, stream, (const SensorArg*)nullptr, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_linearize(const vus_ba_problem* P, const double* poses, const double* points, double* W,
                                double* V, double* gl, double* Hpp, double* gp, double* err, double* work,
                                void* stream) {
  return LinearizeOp<VUS_LOSS_GAUSSIAN>::run(0.0, P, poses, points, W, V, gl, Hpp, gp, err, work, stream, nullptr, nullptr);
}

extern "C" int vus_ba_linearize_robust(const vus_ba_problem* P, const double* poses, const double* points, double* W,
                                       double* V, double* gl, double* Hpp, double* gp, double* err, double* work,
                                       void* stream, const vus_ba_loss* loss) {
  if (int rc = check_loss(loss)) return rc;
  return dispatch_loss<LinearizeOp>(loss, P, poses, points, W, V, gl, Hpp, gp, err, work, stream, (const SensorArg*)nullptr, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_stereo_weights(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses,
                                     const double* points, double* w, void* stream) {
  if (int rc = check_loss(loss)) return rc;
  return dispatch_loss<WeightsOp>(loss, P, poses, points, w, stream, (const SensorArg*)nullptr, (const MonoArg*)nullptr);
}

// ---------------------------------------------------------------------------------------------
// body_P_sensor (include/vus_sensor.h): one set of entry points for the Gaussian and the robust models
namespace {
const vus_ba_loss kGaussianLoss = {VUS_LOSS_GAUSSIAN, 0.0};

// (loss or the Gaussian model for NULL, the kernels' form of the extrinsic), both validated
int sensor_args(const vus_ba_loss*& loss, const vus_ba_sensor* sensor, SensorArg& S) {
  if (!loss) loss = &kGaussianLoss;
  if (int rc = check_loss(loss)) return rc;
  return make_sensor(sensor, S);
}
}  // namespace

extern "C" int vus_ba_error_sensor(const vus_ba_problem* P, const double* poses, const double* points, double* err,
                                   double* work, void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor) {
  SensorArg S;
  if (int rc = sensor_args(loss, sensor, S)) return rc;
  return dispatch_loss<ErrorOp>(loss, P, poses, points, err, work, stream, (const SensorArg*)&S, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_linearize_sensor(const vus_ba_problem* P, const double* poses, const double* points, double* W,
                                       double* V, double* gl, double* Hpp, double* gp, double* err, double* work,
                                       void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor) {
  SensorArg S;
  if (int rc = sensor_args(loss, sensor, S)) return rc;
  return dispatch_loss<LinearizeOp>(loss, P, poses, points, W, V, gl, Hpp, gp, err, work, stream, (const SensorArg*)&S, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_stereo_weights_sensor(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses,
                                            const double* points, double* w, void* stream, const vus_ba_sensor* sensor) {
  SensorArg S;
  if (int rc = sensor_args(loss, sensor, S)) return rc;
  return dispatch_loss<WeightsOp>(loss, P, poses, points, w, stream, (const SensorArg*)&S, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_schur(const vus_ba_problem* P, const vus_ba_tiles* T, double lambda, const double* W, const double* V,
                            const double* gl, const double* Hpp, const double* gp, double* Vinv, double* Y, double* Sband,
                            int band_nodes, double* gs, int* counter, void* stream) {
  if (int rc = check_problem(P)) return rc;
  VUS_REQUIRE(T != nullptr, "tile structure is null");
  const int nP = P->n_poses, nL = P->n_points, nO = P->n_obs;
  const int ps = pose_stride(*P);
  VUS_REQUIRE(Hpp && gp && Sband && gs && counter, "null buffer");
  VUS_REQUIRE((V && gl && Vinv) || !nL, "null landmark buffer");
  VUS_REQUIRE(W || !nO, "null observation buffer");
  VUS_REQUIRE(lambda >= 0.0, "lambda=%g", lambda);
  VUS_REQUIRE(T->band >= 0 && T->n_tiles == (nP + 7) / 8 && T->n_units == T->n_tiles * ((T->band + 7) / 8 + 1) && T->n_entries >= 0,
              "tile structure of another problem: band=%d tiles=%d units=%d", T->band, T->n_tiles, T->n_units);
  VUS_REQUIRE(band_nodes >= ps * T->band && band_nodes < ps * nP + 1, "band_nodes=%d against %d poses of tile band, %d nodes",
              band_nodes, T->band, ps * nP);
  VUS_REQUIRE(T->unit_ptr && T->order && (T->entries || T->n_entries == 0), "tile lists are null");
  hipStream_t st = vus::as_stream(stream);
  // With velocity nodes between the poses (ps = 2) the blocks the tile pairs do not cover belong to the inertial
  // factors and start from zero.  With ps = 1 every stored block (i, k), 0 <= k <= i, i - k <= band_nodes, within the
  // pose distances the units reach (tile distances up to ceil(T->band / 8): 8 ceil(T->band / 8) poses) is WRITTEN by
  // its tile pair (nothing is accumulated into); a wider storage band is zeroed first, since no landmark spans the
  // blocks beyond.  The slots left of pose 0 (k < 0) of the first band rows are never read by the solvers
  // (csrc/band_index.h masks them) and only kept finite.
  const bool beyond_units = band_nodes > 8 * ((T->band + 7) / 8);
  if (ps > 1 || beyond_units)
    VUS_CHECK_HIP(hipMemsetAsync(Sband, 0, sizeof(double) * 36 * (size_t)nP * ps * (band_nodes + 1), st));
  if (ps > 1)
    VUS_CHECK_HIP(hipMemsetAsync(gs, 0, sizeof(double) * 6 * (size_t)nP * ps, st));
  else if (band_nodes > 0 && !beyond_units)
    band_head_zero_kernel<<<min(band_nodes, nP), 256, 0, st>>>(Sband, nP, band_nodes);
  VUS_CHECK_HIP(hipMemsetAsync(counter, 0, sizeof(int), st));
  if (nL > 0) vinv_kernel<<<cdiv(nL, 256), 256, 0, st>>>(nL, lambda, V, Vinv);
  if (nO > 0 && Y != nullptr) ymul_kernel<<<cdiv(nO, 256), 256, 0, st>>>(*P, W, Vinv, Y);   // optional output only
  constexpr int lds = ST_WAVES * ST_WAVE_DOUBLES * (int)sizeof(double);
  // (kernel, device) attribute: set per call -- a host-side table write -- instead of once per process
  VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(schur_tiles_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int n_cu = device_cu_count();
  if (n_cu < 8) n_cu = 256;
  int wg = 2 * n_cu;                 // persistent: two workgroups per CU is what their LDS admits
  if (wg > T->n_units) wg = T->n_units;
  schur_tiles_kernel<<<wg, 64 * ST_WAVES, lds, st>>>(*T, nP, ps, band_nodes, lambda, W, Vinv, Hpp, gl, gp, Sband, gs, counter);
  VUS_CHECK_LAUNCH("ba_schur");
  return VUS_OK;
}

extern "C" int vus_ba_add_diag(double* Sband, int n_poses, int band, double value, void* stream) {
  VUS_REQUIRE(Sband != nullptr, "Sband is null");
  VUS_REQUIRE(n_poses >= 1 && band >= 0, "n_poses=%d band=%d", n_poses, band);
  add_diag_kernel<<<cdiv(6ll * n_poses, 256), 256, 0, vus::as_stream(stream)>>>(Sband, n_poses, band, value);
  VUS_CHECK_LAUNCH("ba_add_diag");
  return VUS_OK;
}

extern "C" int vus_ba_backsub(const vus_ba_problem* P, const double* W, const double* Vinv, const double* gl,
                              const double* dp, double* dl, void* stream) {
  if (int rc = check_problem(P)) return rc;
  VUS_REQUIRE(dp != nullptr, "null buffer");
  VUS_REQUIRE((Vinv && gl && dl) || !P->n_points, "null landmark buffer");
  VUS_REQUIRE(W || !P->n_obs, "null observation buffer");
  if (P->n_points > 0)
    backsub_kernel<<<cdiv(P->n_points, 4), 256, 0, vus::as_stream(stream)>>>(*P, W, Vinv, gl, dp, dl);
  VUS_CHECK_LAUNCH("ba_backsub");
  return VUS_OK;
}

extern "C" int vus_ba_eval_step(const vus_ba_problem* P, const double* poses, const double* points, const double* dp,
                                const double* dl, double* new_poses, double* new_points, double* out, double* work,
                                void* stream) {
  return EvalStepOp<VUS_LOSS_GAUSSIAN>::run(0.0, P, poses, points, dp, dl, new_poses, new_points, out, work, stream, nullptr, nullptr);
}

extern "C" int vus_ba_eval_step_robust(const vus_ba_problem* P, const double* poses, const double* points,
                                       const double* dp, const double* dl, double* new_poses, double* new_points,
                                       double* out, double* work, void* stream, const vus_ba_loss* loss) {
  if (int rc = check_loss(loss)) return rc;
  return dispatch_loss<EvalStepOp>(loss, P, poses, points, dp, dl, new_poses, new_points, out, work, stream,
                                   (const SensorArg*)nullptr, (const MonoArg*)nullptr);
}

extern "C" int vus_ba_eval_step_sensor(const vus_ba_problem* P, const double* poses, const double* points,
                                       const double* dp, const double* dl, double* new_poses, double* new_points,
                                       double* out, double* work, void* stream, const vus_ba_loss* loss,
                                       const vus_ba_sensor* sensor) {
  SensorArg S;
  if (int rc = sensor_args(loss, sensor, S)) return rc;
  return dispatch_loss<EvalStepOp>(loss, P, poses, points, dp, dl, new_poses, new_points, out, work, stream,
                                   (const SensorArg*)&S, (const MonoArg*)nullptr);
}

// ---------------------------------------------------------------------------------------------
// monocular projection factors next to the stereo ones (include/vus_mono.h): the arguments of the `_sensor` forms, the
// extrinsic optional, and the descriptor of the mono observations
namespace {
// (loss or Gaussian for NULL, the extrinsic or none for NULL, the mono descriptor), all validated; Sp = &S or nullptr
int mixed_args(const vus_ba_problem* P, const vus_ba_loss*& loss, const vus_ba_sensor* sensor, const vus_ba_mono* mono,
               SensorArg& S, const SensorArg*& Sp, MonoArg& M) {
  if (!loss) loss = &kGaussianLoss;
  if (int rc = check_loss(loss)) return rc;
  Sp = nullptr;
  if (sensor) {
    if (int rc = make_sensor(sensor, S)) return rc;
    Sp = &S;
  }
  return make_mono(P, mono, M);
}
}  // namespace

extern "C" int vus_ba_error_mixed(const vus_ba_problem* P, const double* poses, const double* points, double* err,
                                  double* work, void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor,
                                  const vus_ba_mono* mono) {
  SensorArg S;
  const SensorArg* Sp;
  MonoArg M;
  if (int rc = mixed_args(P, loss, sensor, mono, S, Sp, M)) return rc;
  return dispatch_loss<ErrorOp>(loss, P, poses, points, err, work, stream, Sp, (const MonoArg*)&M);
}

extern "C" int vus_ba_linearize_mixed(const vus_ba_problem* P, const double* poses, const double* points, double* W,
                                      double* V, double* gl, double* Hpp, double* gp, double* err, double* work,
                                      void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor,
                                      const vus_ba_mono* mono) {
  SensorArg S;
  const SensorArg* Sp;
  MonoArg M;
  if (int rc = mixed_args(P, loss, sensor, mono, S, Sp, M)) return rc;
  return dispatch_loss<LinearizeOp>(loss, P, poses, points, W, V, gl, Hpp, gp, err, work, stream, Sp, (const MonoArg*)&M);
}

extern "C" int vus_ba_eval_step_mixed(const vus_ba_problem* P, const double* poses, const double* points,
                                      const double* dp, const double* dl, double* new_poses, double* new_points,
                                      double* out, double* work, void* stream, const vus_ba_loss* loss,
                                      const vus_ba_sensor* sensor, const vus_ba_mono* mono) {
  SensorArg S;
  const SensorArg* Sp;
  MonoArg M;
  if (int rc = mixed_args(P, loss, sensor, mono, S, Sp, M)) return rc;
  return dispatch_loss<EvalStepOp>(loss, P, poses, points, dp, dl, new_poses, new_points, out, work, stream, Sp,
                                   (const MonoArg*)&M);
}

extern "C" int vus_ba_stereo_weights_mixed(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses,
                                           const double* points, double* w, void* stream, const vus_ba_sensor* sensor,
                                           const vus_ba_mono* mono) {
  SensorArg S;
  const SensorArg* Sp;
  MonoArg M;
  if (int rc = mixed_args(P, loss, sensor, mono, S, Sp, M)) return rc;
  return dispatch_loss<WeightsOp>(loss, P, poses, points, w, stream, Sp, (const MonoArg*)&M);
}
