// nav.hip -- inertial factors for gfx950, in both node layouts: gtsam.ImuFactor over
// preintegrated measurements (reference batch.py:237-239,289-293), the DVL velocity factor (batch.py:196-250, with the
// correct Jacobians), PriorFactorVector on velocities (batch.py:282) and, with one bias per keyframe,
// BetweenFactorConstantBias and PriorFactorConstantBias.  O(#keyframes) work next to the O(#observations) stereo
// kernels of ba.hip.
//
// Two node layouts (vus_ba_problem.pose_stride), one set of factor kernels templated on the layout:
//   SharedBias (stride 2, include/vus.h vus_nav_*): node 2i = X(i), node 2i+1 = V(i) padded to 6 dims (dims 3..5 are
//     inert: unit diagonal, zero right-hand side); the shared bias B(0) is a 6-wide BORDER of the reduced camera
//     system, eliminated after the band solve with 7 right-hand sides.  Snav has 4 block diagonals.
//   PerKeyframeBias (stride 3, include/vus_nav_bias.h vus_navb_*): node 3i = X(i), 3i+1 = V(i) padded to 6, 3i+2 =
//     B(i).  No border: each lambda trial is one single-right-hand-side band solve.  An ImuFactor's columns land on
//     nodes 3i .. 3i+4, so Snav has 5 block diagonals.
//
// Factors are evaluated one per thread.  Their J^T J blocks on the camera side go in with f64 atomics (a block receives
// a handful of addends, so two runs agree to ~1e-16 relative, not bitwise).  With the shared bias, the bias-bias block
// and the bias gradient, which every IMU factor touches, are written per factor and reduced in a fixed order, and the
// velocity priors are added by one sequential thread.
#include <cmath>
#include <cstring>
#include <vector>
#include "vus_common.h"
#include "imu_device.h"   // the ImuFactor arithmetic (and through it se3_device.h): one copy for every inertial unit

namespace {

// ---- the two node layouts ---------------------------------------------------------------------------------------------
// ImuFactor columns (pose_i, vel_i, pose_j, vel_j, bias) -> (node, dim); node -1 = the shared-bias border
struct SharedBias {
  using Factors = vus_nav_factors;
  static constexpr int STRIDE = 2, SDIAG = 4;   // node stride, block diagonals of Snav
  static constexpr bool BORDER = true;          // bias columns -> border; their step in mode 2 is db
  __device__ static const double* imu_bias(const double* bias, int) { return bias; }
  __device__ static void imu_col(int c, int i, int j, int& node, int& dim) {
    if (c < 6) { node = 2 * i; dim = c; }
    else if (c < 9) { node = 2 * i + 1; dim = c - 6; }
    else if (c < 15) { node = 2 * j; dim = c - 9; }
    else if (c < 18) { node = 2 * j + 1; dim = c - 15; }
    else { node = -1; dim = c - 18; }
  }
};
struct PerKeyframeBias {
  using Factors = vus_navb_factors;
  static constexpr int STRIDE = 3, SDIAG = 5;
  static constexpr bool BORDER = false;         // bias columns -> node 3i+2; their step in mode 2 is dc
  __device__ static const double* imu_bias(const double* biases, int i) { return biases + 6 * (size_t)i; }
  __device__ static void imu_col(int c, int i, int, int& node, int& dim) {   // j = i + 1, checked on the host
    if (c < 6) { node = 3 * i; dim = c; }
    else if (c < 9) { node = 3 * i + 1; dim = c - 6; }
    else if (c < 15) { node = 3 * i + 3; dim = c - 9; }
    else if (c < 18) { node = 3 * i + 4; dim = c - 15; }
    else { node = 3 * i + 2; dim = c - 18; }
  }
};

// error partials that follow the IMU and DVL ones: velocity priors, plus the bias factors of the per-keyframe layout
inline int n_diag(const vus_nav_factors& N) { return N.n_vprior; }
inline int n_diag(const vus_navb_factors& N) { return N.n_vprior + N.n_bbetween + N.n_bprior; }

// scratch record of one evaluated factor: whitened Jacobian rows followed by the whitened residual
constexpr int IMU_REC = 9 * 25;   // Jw[9][24] | rw[9] stored as row a: 24 J entries + 1 residual
constexpr int DVL_REC = 3 * 10;   // Jw[3][9]  | rw[3]
constexpr int NAV_BIAS_PART = 42; // shared bias: 36 (Sbb) + 6 (gb) per IMU factor

// mode 0: Jacobians + residual into the scratch records;  mode 1: error only (part[f]);
// mode 2: linearised error 0.5 |rw + Jw d|^2 with d from the node step dc (and db for the border) (part[f]).
template <class L>
__global__ void nav_imu_kernel(typename L::Factors N, const double* __restrict__ poses, const double* __restrict__ vels,
                               const double* __restrict__ bias, const double* __restrict__ dc,
                               const double* __restrict__ db, double* __restrict__ rec, double* __restrict__ part,
                               int mode) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N.n_imu) return;
  const int i = N.imu_i[f], j = N.imu_j[f];
  double r[9], J[9 * 24];
  imu_factor(poses + 12 * (size_t)i, vels + 3 * (size_t)i, poses + 12 * (size_t)j, vels + 3 * (size_t)j,
             L::imu_bias(bias, i), N.imu_pim + PIM_N * (size_t)f, N.gravity, r, mode == 1 ? nullptr : J);
  const double* W = N.imu_W + 81 * (size_t)f;
  double e = 0.0;
  for (int a = 0; a < 9; ++a) {
    double rw = 0.0;
    for (int k = 0; k < 9; ++k) rw += W[9 * a + k] * r[k];
    if (mode != 1) {
      double* out = rec + IMU_REC * (size_t)f + 25 * a;
      for (int c = 0; c < 24; ++c) {
        double jw = 0.0;
        for (int k = 0; k < 9; ++k) jw += W[9 * a + k] * J[24 * k + c];
        if (mode == 0) out[c] = jw;
        else {
          int node, dim;
          L::imu_col(c, i, j, node, dim);
          rw += jw * (L::BORDER && node < 0 ? db[dim] : dc[6 * (size_t)node + dim]);
        }
      }
      if (mode == 0) out[24] = rw;
    }
    e += 0.5 * rw * rw;
  }
  part[f] = e;
}

template <class L>
__global__ void nav_dvl_kernel(typename L::Factors N, const double* __restrict__ poses, const double* __restrict__ vels,
                               const double* __restrict__ dc, double* __restrict__ rec, double* __restrict__ part,
                               int mode) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N.n_dvl) return;
  const int i = N.dvl_pose[f];
  const double* T = poses + 12 * (size_t)i;
  const double* m = N.dvl_meas + 3 * (size_t)f;
  const double w = N.dvl_w[f];
  double Rm[3], X[9], M[9];
  mv(T, m, Rm);
  skew(m, X);
  mm(T, X, M);   // R [m]x
  double e = 0.0;
  for (int a = 0; a < 3; ++a) {
    double rw = w * (Rm[a] - vels[3 * (size_t)i + a]);
    double Jw[9];
    for (int b = 0; b < 3; ++b) { Jw[b] = -w * M[3 * a + b]; Jw[3 + b] = 0.0; Jw[6 + b] = (a == b) ? -w : 0.0; }
    if (mode == 0) {
      double* out = rec + DVL_REC * (size_t)f + 10 * a;
      for (int c = 0; c < 9; ++c) out[c] = Jw[c];
      out[9] = rw;
    } else if (mode == 2) {
      for (int c = 0; c < 6; ++c) rw += Jw[c] * dc[6 * (size_t)(L::STRIDE * i) + c];
      for (int c = 0; c < 3; ++c) rw += Jw[6 + c] * dc[6 * (size_t)(L::STRIDE * i + 1) + c];
    }
    e += 0.5 * rw * rw;
  }
  part[f] = e;
}

// shared bias: error of the velocity priors (accumulated by nav_vprior_accumulate_kernel)
__global__ void nav_vprior_kernel(vus_nav_factors N, const double* __restrict__ vels, const double* __restrict__ dc,
                                  double* __restrict__ part, int mode) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N.n_vprior) return;
  const int i = N.vprior_idx[f];
  double e = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double w = N.vprior_w[3 * (size_t)f + k];
    double r = w * (vels[3 * (size_t)i + k] - N.vprior_v[3 * (size_t)f + k]);
    if (mode == 2) r += w * dc[6 * (size_t)(2 * i + 1) + k];
    e += 0.5 * r * r;
  }
  part[f] = e;
}

// per-keyframe bias, the diagonal factors: velocity priors (3 coordinates on node 3i+1), bias between-factors (6
// coordinates, nodes 3i+2 and 3i+5), bias priors (6 coordinates on node 3i+2).  One thread per factor; mode 0 also
// accumulates (atomics).
__global__ void navb_diag_kernel(vus_navb_factors N, const double* __restrict__ vels, const double* __restrict__ biases,
                                 const double* __restrict__ dc, double* __restrict__ Snav, double* __restrict__ gnav,
                                 double* __restrict__ part, int mode) {
  constexpr int NB_SDIAG = PerKeyframeBias::SDIAG;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nv = N.n_vprior, nb = N.n_bbetween;
  if (t >= nv + nb + N.n_bprior) return;
  double e = 0.0;
  if (t < nv) {
    const int i = N.vprior_idx[t];
    const size_t node = 3 * (size_t)i + 1;
    for (int k = 0; k < 3; ++k) {
      const double w = N.vprior_w[3 * (size_t)t + k];
      double r = w * (vels[3 * (size_t)i + k] - N.vprior_v[3 * (size_t)t + k]);
      if (mode == 0) {
        unsafeAtomicAdd(&Snav[36 * (node * NB_SDIAG) + 7 * k], w * w);
        unsafeAtomicAdd(&gnav[6 * node + k], w * r);
      } else if (mode == 2) {
        r += w * dc[6 * node + k];
      }
      e += 0.5 * r * r;
    }
  } else if (t < nv + nb) {
    const int f = t - nv;
    const int i = N.bb_i[f], j = N.bb_j[f];
    const size_t ni = 3 * (size_t)i + 2, nj = 3 * (size_t)j + 2;
    for (int k = 0; k < 6; ++k) {
      const double w = N.bb_w[6 * (size_t)f + k];
      double r = w * (biases[6 * (size_t)j + k] - biases[6 * (size_t)i + k] - N.bb_meas[6 * (size_t)f + k]);
      if (mode == 0) {
        unsafeAtomicAdd(&Snav[36 * (ni * NB_SDIAG) + 7 * k], w * w);
        unsafeAtomicAdd(&Snav[36 * (nj * NB_SDIAG) + 7 * k], w * w);
        unsafeAtomicAdd(&Snav[36 * (nj * NB_SDIAG + (nj - ni)) + 7 * k], -w * w);
        unsafeAtomicAdd(&gnav[6 * ni + k], -w * r);
        unsafeAtomicAdd(&gnav[6 * nj + k], w * r);
      } else if (mode == 2) {
        r += w * (dc[6 * nj + k] - dc[6 * ni + k]);
      }
      e += 0.5 * r * r;
    }
  } else {
    const int f = t - nv - nb;
    const int i = N.bp_idx[f];
    const size_t node = 3 * (size_t)i + 2;
    for (int k = 0; k < 6; ++k) {
      const double w = N.bp_w[6 * (size_t)f + k];
      double r = w * (biases[6 * (size_t)i + k] - N.bp_mean[6 * (size_t)f + k]);
      if (mode == 0) {
        unsafeAtomicAdd(&Snav[36 * (node * NB_SDIAG) + 7 * k], w * w);
        unsafeAtomicAdd(&gnav[6 * node + k], w * r);
      } else if (mode == 2) {
        r += w * dc[6 * node + k];
      }
      e += 0.5 * r * r;
    }
  }
  part[t] = e;
}

// One workgroup per IMU factor: thread t < 576 owns entry (c1, c2) of the 24x24 block, threads 576..599 the gradient.
// Camera-side blocks go in with f64 atomics.  Shared bias: the node-bias coupling goes to Scb (atomics); the bias-bias
// block and the bias gradient, which EVERY IMU factor touches, are written per factor to bias_part and reduced in a
// fixed order afterwards (nav_bias_reduce_kernel).
template <class L>
__global__ __launch_bounds__(640) void nav_accumulate_imu_kernel(typename L::Factors N, const double* __restrict__ rec_imu,
                                                                 double* __restrict__ Snav, double* __restrict__ gnav,
                                                                 double* __restrict__ Scb,
                                                                 double* __restrict__ bias_part) {
  const int t = threadIdx.x, f = blockIdx.x;
  const int i = N.imu_i[f], j = N.imu_j[f];
  const double* R = rec_imu + IMU_REC * (size_t)f;
  if (t < 576) {
    const int c1 = t / 24, c2 = t - 24 * c1;
    int n1, d1, n2, d2;
    L::imu_col(c1, i, j, n1, d1);
    L::imu_col(c2, i, j, n2, d2);
    if (n1 < n2) return;                       // the upper triangle is the transpose of what the lower one stores
    double h = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) h += R[25 * a + c1] * R[25 * a + c2];
    if (L::BORDER && n2 < 0) {
      if (n1 >= 0) unsafeAtomicAdd(&Scb[36 * (size_t)n1 + 6 * d1 + d2], h);
      else bias_part[NAV_BIAS_PART * (size_t)f + 6 * d1 + d2] = h;
    } else if (!L::BORDER || n1 - n2 < L::SDIAG) {   // shared bias: imu_j is not checked on the host
      unsafeAtomicAdd(&Snav[36 * ((size_t)n1 * L::SDIAG + (n1 - n2)) + 6 * d1 + d2], h);
    }
  } else if (t < 600) {
    const int c = t - 576;
    double gsum = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) gsum += R[25 * a + c] * R[25 * a + 24];
    int n1, d1;
    L::imu_col(c, i, j, n1, d1);
    if (L::BORDER && n1 < 0) bias_part[NAV_BIAS_PART * (size_t)f + 36 + d1] = gsum;
    else unsafeAtomicAdd(&gnav[6 * (size_t)n1 + d1], gsum);
  }
}

__global__ __launch_bounds__(64) void nav_bias_reduce_kernel(int n_imu, const double* __restrict__ bias_part,
                                                            double* __restrict__ Sbb, double* __restrict__ gb) {
  const int e = blockIdx.x, lane = threadIdx.x;
  double acc = 0.0;
  for (int f = lane; f < n_imu; f += 64) acc += bias_part[NAV_BIAS_PART * (size_t)f + e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    if (e < 36) Sbb[e] = acc;
    else gb[e - 36] = acc;
  }
}

template <class L>
__global__ __launch_bounds__(128) void nav_accumulate_dvl_kernel(typename L::Factors N, const double* __restrict__ rec_dvl,
                                                                 double* __restrict__ Snav, double* __restrict__ gnav) {
  constexpr int S = L::STRIDE;
  const int t = threadIdx.x, f = blockIdx.x;
  const int i = N.dvl_pose[f];
  const double* R = rec_dvl + DVL_REC * (size_t)f;
  if (t < 81) {
    const int c1 = t / 9, c2 = t - 9 * c1;
    const int n1 = c1 < 6 ? S * i : S * i + 1, d1 = c1 < 6 ? c1 : c1 - 6;
    const int n2 = c2 < 6 ? S * i : S * i + 1, d2 = c2 < 6 ? c2 : c2 - 6;
    if (n1 < n2) return;
    double h = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) h += R[10 * a + c1] * R[10 * a + c2];
    unsafeAtomicAdd(&Snav[36 * ((size_t)n1 * L::SDIAG + (n1 - n2)) + 6 * d1 + d2], h);
  } else if (t < 90) {
    const int c = t - 81;
    double gsum = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) gsum += R[10 * a + c] * R[10 * a + 9];
    const int n1 = c < 6 ? S * i : S * i + 1, d1 = c < 6 ? c : c - 6;
    unsafeAtomicAdd(&gnav[6 * (size_t)n1 + d1], gsum);
  }
}

// shared bias: velocity priors are diagonal; run after the accumulate kernels (same stream)
__global__ void nav_vprior_accumulate_kernel(vus_nav_factors N, const double* __restrict__ vels,
                                             double* __restrict__ Snav, double* __restrict__ gnav) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int f = 0; f < N.n_vprior; ++f) {   // several priors on one velocity are legal: keep it sequential
    const int node = 2 * N.vprior_idx[f] + 1;
    for (int k = 0; k < 3; ++k) {
      const double w = N.vprior_w[3 * (size_t)f + k];
      const double r = w * (vels[3 * (size_t)N.vprior_idx[f] + k] - N.vprior_v[3 * (size_t)f + k]);
      Snav[36 * ((size_t)node * 4) + 7 * k] += w * w;
      gnav[6 * (size_t)node + k] += w * r;
    }
  }
}

__global__ void nav_assemble_kernel(int n_nodes, int band, double lambda, const double* __restrict__ Snav,
                                    const double* __restrict__ Scb, const double* __restrict__ gnav,
                                    double* __restrict__ Sband, double* __restrict__ gs, double* __restrict__ rhs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * n_nodes) return;
  const int node = t / 36, e = t - 36 * node;
  const int smax = min(3, band);
  for (int s = 0; s <= smax; ++s) {
    double v = Snav[36 * ((size_t)node * 4 + s) + e];
    if (s == 0 && (node & 1) && e % 7 == 0) v += (e / 7 < 3) ? lambda : 1.0;   // velocity node: damping / padding
    Sband[36 * ((size_t)node * (band + 1) + s) + e] += v;
  }
  if (e < 6) {
    const size_t k = 6 * (size_t)node + e;
    const double g = gs[k] + gnav[k];
    gs[k] = g;
    rhs[k] = -g;
  }
  // columns 1..6 of the right-hand sides: the bias coupling, entry (6*node + d, q) = Scb[node][d][q]
  const int d = e / 6, q = e - 6 * d;
  rhs[(size_t)(1 + q) * 6 * n_nodes + 6 * (size_t)node + d] = Scb[t];
}

__global__ void navb_assemble_kernel(int n_nodes, int band, double lambda, const double* __restrict__ Snav,
                                     const double* __restrict__ gnav, double* __restrict__ Sband, double* __restrict__ gs) {
  constexpr int NB_SDIAG = PerKeyframeBias::SDIAG;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * n_nodes) return;
  const int node = t / 36, e = t - 36 * node;
  const int kind = node % 3;                  // 0 pose (damped by vus_ba_schur), 1 velocity, 2 bias
  const int smax = min(NB_SDIAG - 1, min(band, node));
  for (int s = 0; s <= smax; ++s) {
    double v = Snav[36 * ((size_t)node * NB_SDIAG + s) + e];
    if (s == 0 && e % 7 == 0) {
      if (kind == 1) v += (e / 7 < 3) ? lambda : 1.0;   // velocity node: damping / padding
      else if (kind == 2) v += lambda;
    }
    Sband[36 * ((size_t)node * (band + 1) + s) + e] += v;
  }
  if (e < 6) {
    const size_t k = 6 * (size_t)node + e;
    gs[k] += gnav[k];
  }
}

// shared bias: (Sbb + lambda I - Scb^T Z) db = -gb - Scb^T z0;  dc = z0 - Z db.   One workgroup.
__global__ __launch_bounds__(1024) void nav_border_kernel(int n_nodes, const double* __restrict__ rhs,
                                                          const double* __restrict__ Scb, const double* __restrict__ Sbb,
                                                          const double* __restrict__ gb, double lambda,
                                                          double* __restrict__ dc, double* __restrict__ db) {
  __shared__ double s_red[16][42];
  __shared__ double s_db[6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = 6 * (size_t)n_nodes;
  double acc[42];   // [a][0..5]: (Scb^T Z)[a][b];  [36 + a]: (Scb^T z0)[a]
#pragma unroll
  for (int k = 0; k < 42; ++k) acc[k] = 0.0;
  for (size_t k = tid; k < n; k += 1024) {
    const size_t node = k / 6;
    const int d = (int)(k - 6 * node);
    const double* c = Scb + 36 * node + 6 * d;   // row d of the node's coupling block = (Scb)[k][0..5]
    const double z0 = rhs[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      acc[36 + a] += c[a] * z0;
#pragma unroll
      for (int b = 0; b < 6; ++b) acc[6 * a + b] += c[a] * rhs[(size_t)(1 + b) * n + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 42; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double M[36], v[6];
    for (int k = 0; k < 42; ++k) {
      double t = 0.0;
      for (int w = 0; w < 16; ++w) t += s_red[w][k];
      if (k < 36) M[k] = Sbb[k] + ((k % 7 == 0) ? lambda : 0.0) - t;
      else v[k - 36] = -gb[k - 36] - t;
    }
    // Cholesky of the 6x6 SPD border block
    for (int c = 0; c < 6; ++c) {
      double sdiag = M[7 * c];
      for (int k = 0; k < c; ++k) sdiag -= M[6 * c + k] * M[6 * c + k];
      const double l = sqrt(sdiag > 0.0 ? sdiag : 1e-300);
      M[7 * c] = l;
      for (int r = c + 1; r < 6; ++r) {
        double tt = M[6 * r + c];
        for (int k = 0; k < c; ++k) tt -= M[6 * r + k] * M[6 * c + k];
        M[6 * r + c] = tt / l;
      }
    }
    for (int r = 0; r < 6; ++r) { double tt = v[r]; for (int k = 0; k < r; ++k) tt -= M[6 * r + k] * v[k]; v[r] = tt / M[7 * r]; }
    for (int c = 5; c >= 0; --c) { double tt = v[c]; for (int r = c + 1; r < 6; ++r) tt -= M[6 * r + c] * v[r]; v[c] = tt / M[7 * c]; }
    for (int k = 0; k < 6; ++k) { s_db[k] = v[k]; db[k] = v[k]; }
  }
  __syncthreads();
  for (size_t k = tid; k < n; k += 1024) {
    double t = rhs[k];
#pragma unroll
    for (int b = 0; b < 6; ++b) t -= rhs[(size_t)(1 + b) * n + k] * s_db[b];
    dc[k] = t;
  }
}

template <class L>
__global__ void nav_retract_kernel(int n_poses, const double* __restrict__ vels, const double* __restrict__ bias,
                                   const double* __restrict__ dc, const double* __restrict__ db,
                                   double* __restrict__ new_vels, double* __restrict__ new_bias) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 3 * n_poses) new_vels[t] = vels[t] + dc[6 * (size_t)(L::STRIDE * (t / 3) + 1) + t % 3];
  if constexpr (L::BORDER) {
    if (t < 6) new_bias[t] = bias[t] + db[t];
  } else {
    if (t < 6 * n_poses) new_bias[t] = bias[t] + dc[6 * (size_t)(3 * (t / 6) + 2) + t % 6];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the pointer checks of the fields both factor structs share
template <class F>
int check_arrays(const F* N) {
  if (N->n_imu > 0) VUS_REQUIRE(N->imu_i && N->imu_j && N->imu_pim && N->imu_W, "imu arrays are null");
  if (N->n_dvl > 0) VUS_REQUIRE(N->dvl_pose && N->dvl_meas && N->dvl_w, "dvl arrays are null");
  if (N->n_vprior > 0) VUS_REQUIRE(N->vprior_idx && N->vprior_v && N->vprior_w, "velocity prior arrays are null");
  return VUS_OK;
}

// shared bias: sizes and pointers only (no read-back: this runs in every LM trial)
int check_nav(const vus_nav_factors* N, int n_poses) {
  VUS_REQUIRE(N != nullptr, "nav factors are null");
  VUS_REQUIRE(n_poses >= 1 && N->n_imu >= 0 && N->n_dvl >= 0 && N->n_vprior >= 0, "bad sizes");
  return check_arrays(N);
}

// a device index array, read back for the host-side checks
int read_indices(const int* d, int n, std::vector<int>& out) {
  out.resize(n > 0 ? n : 0);
  if (n > 0) VUS_CHECK_HIP(hipMemcpy(out.data(), d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  return VUS_OK;
}

// per-keyframe bias: every size, pointer and index the kernels rely on, checked on the host before anything is launched
int check_navb(const vus_navb_factors* N, int n_poses) {
  VUS_REQUIRE(N != nullptr, "nav factors are null");
  VUS_REQUIRE(n_poses >= 1, "n_poses=%d", n_poses);
  VUS_REQUIRE(N->n_imu >= 0 && N->n_dvl >= 0 && N->n_vprior >= 0 && N->n_bbetween >= 0 && N->n_bprior >= 0,
              "bad sizes: n_imu=%d n_dvl=%d n_vprior=%d n_bbetween=%d n_bprior=%d", N->n_imu, N->n_dvl, N->n_vprior,
              N->n_bbetween, N->n_bprior);
  if (int rc = check_arrays(N)) return rc;
  if (N->n_bbetween > 0) VUS_REQUIRE(N->bb_i && N->bb_j && N->bb_meas && N->bb_w, "bias between-factor arrays are null");
  if (N->n_bprior > 0) VUS_REQUIRE(N->bp_idx && N->bp_mean && N->bp_w, "bias prior arrays are null");
  std::vector<int> a, b;
  if (int rc = read_indices(N->imu_i, N->n_imu, a)) return rc;
  if (int rc = read_indices(N->imu_j, N->n_imu, b)) return rc;
  for (int f = 0; f < N->n_imu; ++f)
    VUS_REQUIRE(a[f] >= 0 && a[f] + 1 < n_poses && b[f] == a[f] + 1,
                "ImuFactor %d joins poses %d and %d: needs j = i + 1 < n_poses=%d", f, a[f], b[f], n_poses);
  if (int rc = read_indices(N->bb_i, N->n_bbetween, a)) return rc;
  if (int rc = read_indices(N->bb_j, N->n_bbetween, b)) return rc;
  for (int f = 0; f < N->n_bbetween; ++f)
    VUS_REQUIRE(a[f] >= 0 && a[f] + 1 < n_poses && b[f] == a[f] + 1,
                "bias between-factor %d joins biases %d and %d: needs bb_j = bb_i + 1 < n_poses=%d", f, a[f], b[f], n_poses);
  const struct { const int* p; int n; const char* what; } one[] = {
      {N->dvl_pose, N->n_dvl, "dvl_pose"}, {N->vprior_idx, N->n_vprior, "vprior_idx"}, {N->bp_idx, N->n_bprior, "bp_idx"}};
  for (const auto& o : one) {
    if (int rc = read_indices(o.p, o.n, a)) return rc;
    for (int f = 0; f < o.n; ++f)
      VUS_REQUIRE(a[f] >= 0 && a[f] < n_poses, "%s[%d]=%d is out of range (n_poses=%d)", o.what, f, a[f], n_poses);
  }
  return VUS_OK;
}

// work layout: [records of the IMU factors | records of the DVL factors | error partials | 8 | bias partials (shared
// bias only, NAV_BIAS_PART per IMU factor)]
template <class F>
long long errors_doubles(const F& N) {
  return (long long)IMU_REC * N.n_imu + (long long)DVL_REC * N.n_dvl + N.n_imu + N.n_dvl + n_diag(N) + 8;
}
struct NavWork {
  double *rec_imu, *rec_dvl, *part;
};
template <class F>
NavWork split_work(const F* N, double* work) {
  NavWork w;
  w.rec_imu = work;
  w.rec_dvl = w.rec_imu + (size_t)IMU_REC * N->n_imu;
  w.part = w.rec_dvl + (size_t)DVL_REC * N->n_dvl;
  return w;
}

// error partials of every factor kind into part[0 .. n_imu + n_dvl + n_diag), reduced into out[0]; mode 0 also writes
// the IMU / DVL records and, per keyframe bias, accumulates the diagonal factors into (Snav, gnav)
template <class L>
int nav_errors(const typename L::Factors* N, const double* poses, const double* vels, const double* bias,
               const double* dc, const double* db, int mode, const NavWork& w, double* Snav, double* gnav, double* out,
               hipStream_t st) {
  const int nd = n_diag(*N);
  if (N->n_imu > 0)
    nav_imu_kernel<L><<<cdiv(N->n_imu, 64), 64, 0, st>>>(*N, poses, vels, bias, dc, db, w.rec_imu, w.part, mode);
  if (N->n_dvl > 0)
    nav_dvl_kernel<L><<<cdiv(N->n_dvl, 64), 64, 0, st>>>(*N, poses, vels, dc, w.rec_dvl, w.part + N->n_imu, mode);
  double* part_diag = w.part + N->n_imu + N->n_dvl;
  if constexpr (L::BORDER) {
    if (nd > 0) nav_vprior_kernel<<<cdiv(nd, 64), 64, 0, st>>>(*N, vels, dc, part_diag, mode);
  } else {
    if (nd > 0) navb_diag_kernel<<<cdiv(nd, 64), 64, 0, st>>>(*N, vels, bias, dc, Snav, gnav, part_diag, mode);
  }
  vus::reduce_partials(w.part, N->n_imu + N->n_dvl + nd, out, st);
  VUS_CHECK_LAUNCH(L::BORDER ? "nav_errors" : "navb_errors");
  return VUS_OK;
}

// new velocities and biases at the step, then the linearised error at the old values (out[0]) and the error at the new
// ones (out[1])
template <class L>
int nav_eval_step(const typename L::Factors* N, int n_poses, const double* poses, const double* vels, const double* bias,
                  const double* dc, const double* db, const double* new_poses, double* new_vels, double* new_bias,
                  double* out, double* work, hipStream_t st) {
  const long long n_retract = L::BORDER ? 3ll * n_poses + 6 : 6ll * n_poses;
  nav_retract_kernel<L><<<cdiv(n_retract, 256), 256, 0, st>>>(n_poses, vels, bias, dc, db, new_vels, new_bias);
  const NavWork w = split_work(N, work);
  if (int rc = nav_errors<L>(N, poses, vels, bias, dc, db, 2, w, nullptr, nullptr, out, st)) return rc;
  return nav_errors<L>(N, new_poses, new_vels, new_bias, nullptr, nullptr, 1, w, nullptr, nullptr, out + 1, st);
}

}  // namespace

// ---- shared bias (include/vus.h) -----------------------------------------------------------------------------------
extern "C" long long vus_nav_work_doubles(const vus_nav_factors* N) {
  if (!N) return 0;
  return errors_doubles(*N) + (long long)NAV_BIAS_PART * N->n_imu;
}

extern "C" int vus_nav_linearize(const vus_nav_factors* N, int n_poses, const double* poses, const double* vels,
                                 const double* bias, double* Snav, double* Scb, double* Sbb, double* gnav, double* gb,
                                 double* err, double* work, void* stream) {
  if (int rc = check_nav(N, n_poses)) return rc;
  VUS_REQUIRE(poses && vels && bias && Snav && Scb && Sbb && gnav && gb && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  const size_t n_nodes = 2 * (size_t)n_poses;
  VUS_CHECK_HIP(hipMemsetAsync(Snav, 0, sizeof(double) * 36 * SharedBias::SDIAG * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(Scb, 0, sizeof(double) * 36 * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(Sbb, 0, sizeof(double) * 36, st));
  VUS_CHECK_HIP(hipMemsetAsync(gnav, 0, sizeof(double) * 6 * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(gb, 0, sizeof(double) * 6, st));
  const NavWork w = split_work(N, work);
  if (int rc = nav_errors<SharedBias>(N, poses, vels, bias, nullptr, nullptr, 0, w, nullptr, nullptr, err, st)) return rc;
  double* bias_part = work + errors_doubles(*N);
  if (N->n_imu > 0) {
    nav_accumulate_imu_kernel<SharedBias><<<N->n_imu, 640, 0, st>>>(*N, w.rec_imu, Snav, gnav, Scb, bias_part);
    nav_bias_reduce_kernel<<<NAV_BIAS_PART, 64, 0, st>>>(N->n_imu, bias_part, Sbb, gb);
  }
  if (N->n_dvl > 0) nav_accumulate_dvl_kernel<SharedBias><<<N->n_dvl, 128, 0, st>>>(*N, w.rec_dvl, Snav, gnav);
  nav_vprior_accumulate_kernel<<<1, 64, 0, st>>>(*N, vels, Snav, gnav);
  VUS_CHECK_LAUNCH("nav_linearize");
  return VUS_OK;
}

extern "C" int vus_nav_assemble(int n_nodes, int band, double lambda, const double* Snav, const double* Scb,
                                const double* gnav, double* Sband, double* gs, double* rhs, void* stream) {
  VUS_REQUIRE(Snav && Scb && gnav && Sband && gs && rhs, "null buffer");
  VUS_REQUIRE(n_nodes >= 2 && (n_nodes & 1) == 0 && band >= 1 && lambda >= 0.0, "n_nodes=%d band=%d lambda=%g", n_nodes,
              band, lambda);
  nav_assemble_kernel<<<cdiv(36ll * n_nodes, 256), 256, 0, vus::as_stream(stream)>>>(n_nodes, band, lambda, Snav, Scb,
                                                                                   gnav, Sband, gs, rhs);
  VUS_CHECK_LAUNCH("nav_assemble");
  return VUS_OK;
}

extern "C" int vus_nav_border_solve(int n_nodes, const double* rhs, const double* Scb, const double* Sbb,
                                    const double* gb, double lambda, double* dc, double* db, void* stream) {
  VUS_REQUIRE(rhs && Scb && Sbb && gb && dc && db, "null buffer");
  VUS_REQUIRE(n_nodes >= 1, "n_nodes=%d", n_nodes);
  nav_border_kernel<<<1, 1024, 0, vus::as_stream(stream)>>>(n_nodes, rhs, Scb, Sbb, gb, lambda, dc, db);
  VUS_CHECK_LAUNCH("nav_border_solve");
  return VUS_OK;
}

extern "C" int vus_nav_eval_step(const vus_nav_factors* N, int n_poses, const double* poses, const double* vels,
                                 const double* bias, const double* dc, const double* db, const double* new_poses,
                                 double* new_vels, double* new_bias, double* out, double* work, void* stream) {
  if (int rc = check_nav(N, n_poses)) return rc;
  VUS_REQUIRE(poses && vels && bias && dc && db && new_poses && new_vels && new_bias && out && work, "null buffer");
  return nav_eval_step<SharedBias>(N, n_poses, poses, vels, bias, dc, db, new_poses, new_vels, new_bias, out, work,
                                   vus::as_stream(stream));
}

extern "C" int vus_nav_error(const vus_nav_factors* N, int n_poses, const double* poses, const double* vels,
                             const double* bias, double* err, double* work, void* stream) {
  if (int rc = check_nav(N, n_poses)) return rc;
  VUS_REQUIRE(poses && vels && bias && err && work, "null buffer");
  return nav_errors<SharedBias>(N, poses, vels, bias, nullptr, nullptr, 1, split_work(N, work), nullptr, nullptr, err,
                                vus::as_stream(stream));
}

// ---- one bias per keyframe (include/vus_nav_bias.h) ---------------------------------------------------------------
extern "C" long long vus_navb_work_doubles(const vus_navb_factors* N) {
  if (!N) return 0;
  return errors_doubles(*N);
}

extern "C" int vus_navb_linearize(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                                  const double* biases, double* Snav, double* gnav, double* err, double* work,
                                  void* stream) {
  VUS_REQUIRE(poses && vels && biases && Snav && gnav && err && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  hipStream_t st = vus::as_stream(stream);
  const size_t n_nodes = 3 * (size_t)n_poses;
  VUS_CHECK_HIP(hipMemsetAsync(Snav, 0, sizeof(double) * 36 * PerKeyframeBias::SDIAG * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(gnav, 0, sizeof(double) * 6 * n_nodes, st));
  const NavWork w = split_work(N, work);
  if (int rc = nav_errors<PerKeyframeBias>(N, poses, vels, biases, nullptr, nullptr, 0, w, Snav, gnav, err, st)) return rc;
  if (N->n_imu > 0)
    nav_accumulate_imu_kernel<PerKeyframeBias><<<N->n_imu, 640, 0, st>>>(*N, w.rec_imu, Snav, gnav, nullptr, nullptr);
  if (N->n_dvl > 0) nav_accumulate_dvl_kernel<PerKeyframeBias><<<N->n_dvl, 128, 0, st>>>(*N, w.rec_dvl, Snav, gnav);
  VUS_CHECK_LAUNCH("navb_linearize");
  return VUS_OK;
}

extern "C" int vus_navb_assemble(int n_nodes, int band, double lambda, const double* Snav, const double* gnav,
                                 double* Sband, double* gs, void* stream) {
  VUS_REQUIRE(Snav && gnav && Sband && gs, "null buffer");
  VUS_REQUIRE(n_nodes >= 3 && n_nodes % 3 == 0, "n_nodes=%d is not 3 * n_poses", n_nodes);
  VUS_REQUIRE(band >= (n_nodes - 1 < 4 ? n_nodes - 1 : 4) && band < n_nodes, "band=%d for %d nodes: needs min(4, n_nodes - 1) "
              "<= band < n_nodes", band, n_nodes);
  VUS_REQUIRE(lambda >= 0.0 && std::isfinite(lambda), "lambda=%g", lambda);
  navb_assemble_kernel<<<cdiv(36ll * n_nodes, 256), 256, 0, vus::as_stream(stream)>>>(n_nodes, band, lambda, Snav, gnav,
                                                                                    Sband, gs);
  VUS_CHECK_LAUNCH("navb_assemble");
  return VUS_OK;
}

extern "C" int vus_navb_eval_step(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                                  const double* biases, const double* dc, const double* new_poses, double* new_vels,
                                  double* new_biases, double* out, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && dc && new_poses && new_vels && new_biases && out && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  return nav_eval_step<PerKeyframeBias>(N, n_poses, poses, vels, biases, dc, nullptr, new_poses, new_vels, new_biases,
                                        out, work, vus::as_stream(stream));
}

extern "C" int vus_navb_error(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                              const double* biases, double* err, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && err && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  return nav_errors<PerKeyframeBias>(N, poses, vels, biases, nullptr, nullptr, 1, split_work(N, work), nullptr, nullptr,
                                     err, vus::as_stream(stream));
}

// ---- host side: IMU preintegration (gtsam does it in C++ inside integrateMeasurement; the Python restatement of it,
// gtsam/imu.py, cost the end-to-end sequence 78 of its 92 ms) ---------------------------------------------------------
namespace {
namespace pim {
constexpr int DT = 0, DR = 1, DP = 10, DV = 13, DR_DBG = 16, DP_DBA = 25, DP_DBG = 34, DV_DBA = 43, DV_DBG = 52, BIAS = 61, COV = 67;

inline void skew(const double* w, double* W) {
  W[0] = 0.0;   W[1] = -w[2]; W[2] = w[1];
  W[3] = w[2];  W[4] = 0.0;   W[5] = -w[0];
  W[6] = -w[1]; W[7] = w[0];  W[8] = 0.0;
}
inline void mul33(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
inline void mul33_tn(const double* A, const double* B, double* C) {      // A^T B
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
// exp(w^) and the right Jacobian of SO(3), with the small-angle branches of gtsam/imu.py
inline void expmap_jr(const double* w, double* R, double* Jr) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9], W2[9];
  skew(w, W);
  mul33(W, W, W2);
  double s1, s2;
  if (th2 <= 2.220446049250313e-16) {
    s1 = 1.0;
    s2 = 0.0;
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + W[i];
  } else {
    const double th = std::sqrt(th2), sh = std::sin(0.5 * th);
    s1 = std::sin(th) / th;
    s2 = 2.0 * sh * sh / th2;
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + s1 * W[i] + s2 * W2[i];
  }
  double a, b;
  if (th2 < 1e-10) {
    a = 0.5 - th2 / 24.0;
    b = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double th = std::sqrt(th2);
    a = s2;                                  // (1 - cos th) / th^2 without the cancellation
    b = (th - std::sin(th)) / (th2 * th);
  }
  for (int i = 0; i < 9; ++i) Jr[i] = (i % 4 == 0 ? 1.0 : 0.0) - a * W[i] + b * W2[i];
}

// Aout [81], Gout [9 x 6], cov2 [81] (may be null), for the 15 x 15 recursion of vus_imu_preintegrate_combined: the sample's
// A and G = [B | C], and a second 9 x 9 covariance that takes the same step A cov2 A^T + Q9 as the record's, sum for sum
void integrate(double* p, const double* smp, const double* acc_cov, const double* gyro_cov, const double* int_cov,
               double* Aout = nullptr, double* Gout = nullptr, double* cov2 = nullptr) {
  const double dt = smp[6];
  const double a[3] = {smp[0] - p[BIAS], smp[1] - p[BIAS + 1], smp[2] - p[BIAS + 2]};
  const double w[3] = {(smp[3] - p[BIAS + 3]) * dt, (smp[4] - p[BIAS + 4]) * dt, (smp[5] - p[BIAS + 5]) * dt};
  double dRinc[9], Jr[9], aX[9], RaX[9];
  expmap_jr(w, dRinc, Jr);
  skew(a, aX);
  double* dR = p + DR;
  mul33(dR, aX, RaX);
  // covariance: A cov A^T + B (acc_cov / dt) B^T + C (gyro_cov / dt) C^T, + int_cov dt on the position block
  double A[81] = {0.0}, Bm[27] = {0.0}, Cm[27] = {0.0};
  for (int i = 0; i < 9; ++i) A[10 * i] = 1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      A[9 * r + c] = dRinc[3 * c + r];
      A[9 * (3 + r) + c] = -0.5 * dt * dt * RaX[3 * r + c];
      A[9 * (6 + r) + c] = -dt * RaX[3 * r + c];
      Bm[3 * (3 + r) + c] = 0.5 * dt * dt * dR[3 * r + c];
      Bm[3 * (6 + r) + c] = dt * dR[3 * r + c];
      Cm[3 * r + c] = dt * Jr[3 * r + c];
    }
  for (int r = 0; r < 3; ++r) A[9 * (3 + r) + 6 + r] = dt;
  if (Aout) std::memcpy(Aout, A, sizeof(A));
  if (Gout)
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 3; ++c) { Gout[6 * r + c] = Bm[3 * r + c]; Gout[6 * r + 3 + c] = Cm[3 * r + c]; }
  auto propagate = [&](double* cov) {      // cov <- A cov A^T + Q9
    double T[81], N[81];
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) {
        double v = 0.0;
        for (int k = 0; k < 9; ++k) v += A[9 * r + k] * cov[9 * k + c];
        T[9 * r + c] = v;
      }
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) {
        double v = 0.0;
        for (int k = 0; k < 9; ++k) v += T[9 * r + k] * A[9 * c + k];
        N[9 * r + c] = v;
      }
    auto add_noise = [&](const double* G, const double* Q) {      // N += G (Q / dt) G^T, G 9x3
      double GQ[27];
      for (int r = 0; r < 9; ++r)
        for (int c = 0; c < 3; ++c) GQ[3 * r + c] = (G[3 * r] * Q[c] + G[3 * r + 1] * Q[3 + c] + G[3 * r + 2] * Q[6 + c]) / dt;
      for (int r = 0; r < 9; ++r)
        for (int c = 0; c < 9; ++c) N[9 * r + c] += GQ[3 * r] * G[3 * c] + GQ[3 * r + 1] * G[3 * c + 1] + GQ[3 * r + 2] * G[3 * c + 2];
    };
    add_noise(Bm, acc_cov);
    add_noise(Cm, gyro_cov);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) N[9 * (3 + r) + 3 + c] += int_cov[3 * r + c] * dt;
    std::memcpy(cov, N, sizeof(N));
  };
  propagate(p + COV);
  if (cov2) propagate(cov2);
  // bias Jacobians, then the deltas (every update uses the OLD dR, dV)
  double t[9], tmp[9];
  mul33(RaX, p + DR_DBG, t);
  for (int i = 0; i < 9; ++i) {
    p[DP_DBA + i] += p[DV_DBA + i] * dt - 0.5 * dt * dt * dR[i];
    p[DP_DBG + i] += p[DV_DBG + i] * dt - 0.5 * dt * dt * t[i];
    p[DV_DBA + i] -= dt * dR[i];
    p[DV_DBG + i] -= dt * t[i];
  }
  mul33_tn(dRinc, p + DR_DBG, tmp);
  for (int i = 0; i < 9; ++i) p[DR_DBG + i] = tmp[i] - dt * Jr[i];
  double Ra[3];
  for (int r = 0; r < 3; ++r) Ra[r] = dR[3 * r] * a[0] + dR[3 * r + 1] * a[1] + dR[3 * r + 2] * a[2];
  for (int r = 0; r < 3; ++r) {
    p[DP + r] += p[DV + r] * dt + 0.5 * dt * dt * Ra[r];
    p[DV + r] += dt * Ra[r];
  }
  mul33(dR, dRinc, tmp);
  std::memcpy(dR, tmp, sizeof(tmp));
  p[DT] += dt;
}

// W = L^-1, cov = L L^T (N x N); W is written only when cov is positive definite
template <int N>
bool whitening(const double* cov, double* W) {
  double L[N * N] = {0.0};
  for (int c = 0; c < N; ++c) {
    double d = cov[(N + 1) * c];
    for (int k = 0; k < c; ++k) d -= L[N * c + k] * L[N * c + k];
    if (!(d > 0.0)) return false;
    L[(N + 1) * c] = std::sqrt(d);
    for (int r = c + 1; r < N; ++r) {
      double v = cov[N * r + c];
      for (int k = 0; k < c; ++k) v -= L[N * r + k] * L[N * c + k];
      L[N * r + c] = v / L[(N + 1) * c];
    }
  }
  for (int c = 0; c < N; ++c)          // column c of L^-1 by forward substitution
    for (int r = 0; r < N; ++r) {
      double v = (r == c) ? 1.0 : 0.0;
      for (int k = 0; k < r; ++k) v -= L[N * r + k] * W[N * k + c];
      W[N * r + c] = v / L[(N + 1) * r];
    }
  return true;
}

// One sample of the 15 x 15 recursion Sigma <- F Sigma F^T + Q, F = [[A, G], [0, I]], around pim::integrate: with
// Sigma = [[S, C], [C^T, V]] the record's own update gives A S A^T + Q9 in ITS summation order (so V = C = 0 leaves the
// record's covariance bit for bit), then S += A C G^T + (A C G^T)^T + G V G^T, C <- A C + G V, V += bias covariances * dt.
void integrate_combined(double* p, double* S15, const double* smp, const double* acc_cov, const double* gyro_cov,
                        const double* int_cov, const double* ba_cov, const double* bg_cov) {
  double S9[81], A[81], G[54];
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 9; ++c) S9[9 * r + c] = S15[15 * r + c];
  integrate(p, smp, acc_cov, gyro_cov, int_cov, A, G, S9);     // the record as vus_imu_preintegrate leaves it; S9 = A S A^T + Q9
  const double dt = smp[6];
  double C[54], V[36], AC[54], GV[54];
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 6; ++c) C[6 * r + c] = S15[15 * r + 9 + c];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) V[6 * r + c] = S15[15 * (9 + r) + 9 + c];
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 6; ++c) {
      double ac = 0.0, gv = 0.0;
      for (int k = 0; k < 9; ++k) ac += A[9 * r + k] * C[6 * k + c];
      for (int k = 0; k < 6; ++k) gv += G[6 * r + k] * V[6 * k + c];
      AC[6 * r + c] = ac;
      GV[6 * r + c] = gv;
    }
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 9; ++c) {
      double x = 0.0;      // (A C G^T)[r][c] + (A C G^T)[c][r] + (G V G^T)[r][c]
      for (int k = 0; k < 6; ++k) x += AC[6 * r + k] * G[6 * c + k] + AC[6 * c + k] * G[6 * r + k] + GV[6 * r + k] * G[6 * c + k];
      S15[15 * r + c] = S9[9 * r + c] + x;
    }
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 6; ++c) S15[15 * r + 9 + c] = S15[15 * (9 + c) + r] = AC[6 * r + c] + GV[6 * r + c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      S15[15 * (9 + r) + 9 + c] += ba_cov[3 * r + c] * dt;
      S15[15 * (12 + r) + 12 + c] += bg_cov[3 * r + c] * dt;
    }
}
}  // namespace pim
}  // namespace

extern "C" int vus_imu_preintegrate(double* pim_rec, const double* samples, int n, const double* acc_cov, const double* gyro_cov,
                                    const double* int_cov, double* whiten) {
  VUS_REQUIRE(pim_rec && acc_cov && gyro_cov && int_cov, "null buffer");
  VUS_REQUIRE(n >= 0 && (samples != nullptr || n == 0), "n=%d", n);
  for (int i = 0; i < n; ++i) {
    VUS_REQUIRE(samples[7 * i + 6] > 0.0, "sample %d: dt=%g is not positive", i, samples[7 * i + 6]);
    pim::integrate(pim_rec, samples + 7 * (size_t)i, acc_cov, gyro_cov, int_cov);
  }
  if (whiten) VUS_REQUIRE(pim::whitening<9>(pim_rec + pim::COV, whiten), "preintegrated covariance is not positive definite");
  return VUS_OK;
}

extern "C" int vus_imu_preintegrate_combined(double* pim_rec, double* cov15, const double* samples, int n, const double* acc_cov,
                                             const double* gyro_cov, const double* int_cov, const double* bias_acc_cov,
                                             const double* bias_omega_cov, double* whiten) {
  VUS_REQUIRE(pim_rec && cov15 && acc_cov && gyro_cov && int_cov && bias_acc_cov && bias_omega_cov, "null buffer");
  VUS_REQUIRE(n >= 0 && (samples != nullptr || n == 0), "n=%d", n);
  for (int i = 0; i < n; ++i) {
    VUS_REQUIRE(samples[7 * i + 6] > 0.0, "sample %d: dt=%g is not positive", i, samples[7 * i + 6]);
    pim::integrate_combined(pim_rec, cov15, samples + 7 * (size_t)i, acc_cov, gyro_cov, int_cov, bias_acc_cov, bias_omega_cov);
  }
  if (whiten) {       // of the RESIDUAL's covariance T cov15 T^T, T = diag(I, dR^T, dR^T, I, I): its p and v rows are in frame j
    const double* dR = pim_rec + pim::DR;
    double T[225] = {0.0}, TS[225], Sr[225];
    for (int k = 0; k < 15; ++k) T[16 * k] = 1.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) T[15 * (3 + r) + 3 + c] = T[15 * (6 + r) + 6 + c] = dR[3 * c + r];
    for (int r = 0; r < 15; ++r)
      for (int c = 0; c < 15; ++c) {
        double v = 0.0;
        for (int k = 0; k < 15; ++k) v += T[15 * r + k] * cov15[15 * k + c];
        TS[15 * r + c] = v;
      }
    for (int r = 0; r < 15; ++r)
      for (int c = 0; c < 15; ++c) {
        double v = 0.0;
        for (int k = 0; k < 15; ++k) v += TS[15 * r + k] * T[15 * c + k];
        Sr[15 * r + c] = v;
      }
    VUS_REQUIRE(pim::whitening<15>(Sr, whiten), "combined preintegrated covariance is not positive definite (a zero bias "
                "covariance leaves its bias block singular)");
  }
  return VUS_OK;
}
