// nav_bias.hip -- inertial factors of graphs with ONE IMU BIAS PER KEYFRAME for gfx950 (include/vus_nav_bias.h):
// ImuFactor(X(i), V(i), X(i+1), V(i+1), B(i)), BetweenFactorConstantBias(B(i), B(i+1)), PriorFactorConstantBias, and
// the DVL factors and velocity priors of nav.hip.  GTSAM's usual visual-inertial graph (ImuFactorsExample).
//
// Node layout (vus_ba_problem.pose_stride = 3): node 3i = X(i), node 3i+1 = V(i) padded to 6 dims (dims 3..5 inert),
// node 3i+2 = B(i).  Every variable is an ordinary band node: no border, and each lambda trial is one
// single-right-hand-side band solve.  An ImuFactor's columns land on nodes 3i .. 3i+4, so the inertial blocks fill the
// block diagonals s = 0..4 of Snav.
//
// Factors are evaluated one per thread (the ImuFactor math is nav_device.h's, shared with nav.hip); their J^T J blocks
// and gradients go in with f64 atomics.  A block receives at most a handful of addends (a bias block: two IMU factors,
// two between-factors, its priors), so two runs agree to ~1e-16 relative, not bitwise.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "nav_device.h"

namespace {

constexpr int NB_IMU_REC = 9 * 25;   // Jw[9][24] | rw[9], row a: 24 J entries + 1 residual (as nav.hip)
constexpr int NB_DVL_REC = 3 * 10;   // Jw[3][9]  | rw[3]
constexpr int NB_SDIAG = 5;          // block diagonals of Snav

// column c of an ImuFactor's 9 x 24 Jacobian (pose_i, vel_i, pose_j, vel_j, bias_i) -> (node, dim); j = i + 1
__device__ __forceinline__ void navb_imu_col(int c, int i, int& node, int& dim) {
  if (c < 6) { node = 3 * i; dim = c; }
  else if (c < 9) { node = 3 * i + 1; dim = c - 6; }
  else if (c < 15) { node = 3 * i + 3; dim = c - 9; }
  else if (c < 18) { node = 3 * i + 4; dim = c - 15; }
  else { node = 3 * i + 2; dim = c - 18; }
}

// mode 0: Jacobians + residual into the scratch records;  mode 1: error only (part[f]);
// mode 2: linearised error 0.5 |rw + Jw d|^2 with d from the node step dc (part[f]).
__global__ void navb_imu_kernel(vus_navb_factors N, const double* __restrict__ poses, const double* __restrict__ vels,
                                const double* __restrict__ biases, const double* __restrict__ dc,
                                double* __restrict__ rec, double* __restrict__ part, int mode) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N.n_imu) return;
  const int i = N.imu_i[f], j = N.imu_j[f];
  double r[9], J[9 * 24];
  imu_factor(poses + 12 * (size_t)i, vels + 3 * (size_t)i, poses + 12 * (size_t)j, vels + 3 * (size_t)j,
             biases + 6 * (size_t)i, N.imu_pim + PIM_N * (size_t)f, N.gravity, r, mode == 1 ? nullptr : J);
  const double* W = N.imu_W + 81 * (size_t)f;
  double e = 0.0;
  for (int a = 0; a < 9; ++a) {
    double rw = 0.0;
    for (int k = 0; k < 9; ++k) rw += W[9 * a + k] * r[k];
    if (mode != 1) {
      double* out = rec + NB_IMU_REC * (size_t)f + 25 * a;
      for (int c = 0; c < 24; ++c) {
        double jw = 0.0;
        for (int k = 0; k < 9; ++k) jw += W[9 * a + k] * J[24 * k + c];
        if (mode == 0) out[c] = jw;
        else {
          int node, dim;
          navb_imu_col(c, i, node, dim);
          rw += jw * dc[6 * (size_t)node + dim];
        }
      }
      if (mode == 0) out[24] = rw;
    }
    e += 0.5 * rw * rw;
  }
  part[f] = e;
}

__global__ void navb_dvl_kernel(vus_navb_factors N, const double* __restrict__ poses, const double* __restrict__ vels,
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
      double* out = rec + NB_DVL_REC * (size_t)f + 10 * a;
      for (int c = 0; c < 9; ++c) out[c] = Jw[c];
      out[9] = rw;
    } else if (mode == 2) {
      for (int c = 0; c < 6; ++c) rw += Jw[c] * dc[6 * (size_t)(3 * i) + c];
      for (int c = 0; c < 3; ++c) rw += Jw[6 + c] * dc[6 * (size_t)(3 * i + 1) + c];
    }
    e += 0.5 * rw * rw;
  }
  part[f] = e;
}

// the diagonal factors: velocity priors (3 coordinates on node 3i+1), bias between-factors (6 coordinates, nodes 3i+2
// and 3i+5), bias priors (6 coordinates on node 3i+2).  One thread per factor; mode 0 also accumulates (atomics).
__global__ void navb_diag_kernel(vus_navb_factors N, const double* __restrict__ vels, const double* __restrict__ biases,
                                 const double* __restrict__ dc, double* __restrict__ Snav, double* __restrict__ gnav,
                                 double* __restrict__ part, int mode) {
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

// One workgroup per ImuFactor: thread t < 576 owns entry (c1, c2) of the 24 x 24 block, threads 576..599 the gradient.
__global__ __launch_bounds__(640) void navb_accumulate_imu_kernel(vus_navb_factors N, const double* __restrict__ rec_imu,
                                                                  double* __restrict__ Snav, double* __restrict__ gnav) {
  const int t = threadIdx.x, f = blockIdx.x;
  const int i = N.imu_i[f];
  const double* R = rec_imu + NB_IMU_REC * (size_t)f;
  if (t < 576) {
    const int c1 = t / 24, c2 = t - 24 * c1;
    int n1, d1, n2, d2;
    navb_imu_col(c1, i, n1, d1);
    navb_imu_col(c2, i, n2, d2);
    if (n1 < n2) return;                       // the upper triangle is the transpose of what the lower one stores
    double h = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) h += R[25 * a + c1] * R[25 * a + c2];
    unsafeAtomicAdd(&Snav[36 * ((size_t)n1 * NB_SDIAG + (n1 - n2)) + 6 * d1 + d2], h);
  } else if (t < 600) {
    const int c = t - 576;
    double gsum = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) gsum += R[25 * a + c] * R[25 * a + 24];
    int n1, d1;
    navb_imu_col(c, i, n1, d1);
    unsafeAtomicAdd(&gnav[6 * (size_t)n1 + d1], gsum);
  }
}

__global__ __launch_bounds__(128) void navb_accumulate_dvl_kernel(vus_navb_factors N, const double* __restrict__ rec_dvl,
                                                                  double* __restrict__ Snav, double* __restrict__ gnav) {
  const int t = threadIdx.x, f = blockIdx.x;
  const int i = N.dvl_pose[f];
  const double* R = rec_dvl + NB_DVL_REC * (size_t)f;
  if (t < 81) {
    const int c1 = t / 9, c2 = t - 9 * c1;
    const int n1 = c1 < 6 ? 3 * i : 3 * i + 1, d1 = c1 < 6 ? c1 : c1 - 6;
    const int n2 = c2 < 6 ? 3 * i : 3 * i + 1, d2 = c2 < 6 ? c2 : c2 - 6;
    if (n1 < n2) return;
    double h = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) h += R[10 * a + c1] * R[10 * a + c2];
    unsafeAtomicAdd(&Snav[36 * ((size_t)n1 * NB_SDIAG + (n1 - n2)) + 6 * d1 + d2], h);
  } else if (t < 90) {
    const int c = t - 81;
    double gsum = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) gsum += R[10 * a + c] * R[10 * a + 9];
    const int n1 = c < 6 ? 3 * i : 3 * i + 1, d1 = c < 6 ? c : c - 6;
    unsafeAtomicAdd(&gnav[6 * (size_t)n1 + d1], gsum);
  }
}

__global__ __launch_bounds__(1024) void navb_reduce_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
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

__global__ void navb_assemble_kernel(int n_nodes, int band, double lambda, const double* __restrict__ Snav,
                                     const double* __restrict__ gnav, double* __restrict__ Sband, double* __restrict__ gs) {
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

__global__ void navb_retract_kernel(int n_poses, const double* __restrict__ vels, const double* __restrict__ biases,
                                    const double* __restrict__ dc, double* __restrict__ new_vels,
                                    double* __restrict__ new_biases) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 3 * n_poses) new_vels[t] = vels[t] + dc[6 * (size_t)(3 * (t / 3) + 1) + t % 3];
  if (t < 6 * n_poses) new_biases[t] = biases[t] + dc[6 * (size_t)(3 * (t / 6) + 2) + t % 6];
}

inline int cdivb(long long a, int b) { return (int)((a + b - 1) / b); }

// a device index array, read back for the host-side checks
int read_indices(const int* d, int n, std::vector<int>& out) {
  out.resize(n > 0 ? n : 0);
  if (n > 0) VUS_CHECK_HIP(hipMemcpy(out.data(), d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  return VUS_OK;
}

// Every size, pointer and index the kernels rely on, checked on the host before anything is launched.
int check_navb(const vus_navb_factors* N, int n_poses) {
  VUS_REQUIRE(N != nullptr, "nav factors are null");
  VUS_REQUIRE(n_poses >= 1, "n_poses=%d", n_poses);
  VUS_REQUIRE(N->n_imu >= 0 && N->n_dvl >= 0 && N->n_vprior >= 0 && N->n_bbetween >= 0 && N->n_bprior >= 0,
              "bad sizes: n_imu=%d n_dvl=%d n_vprior=%d n_bbetween=%d n_bprior=%d", N->n_imu, N->n_dvl, N->n_vprior,
              N->n_bbetween, N->n_bprior);
  if (N->n_imu > 0) VUS_REQUIRE(N->imu_i && N->imu_j && N->imu_pim && N->imu_W, "imu arrays are null");
  if (N->n_dvl > 0) VUS_REQUIRE(N->dvl_pose && N->dvl_meas && N->dvl_w, "dvl arrays are null");
  if (N->n_vprior > 0) VUS_REQUIRE(N->vprior_idx && N->vprior_v && N->vprior_w, "velocity prior arrays are null");
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

struct NavbWork {
  double *rec_imu, *rec_dvl, *part;
};
NavbWork split_work(const vus_navb_factors* N, double* work) {
  NavbWork w;
  w.rec_imu = work;
  w.rec_dvl = w.rec_imu + (size_t)NB_IMU_REC * N->n_imu;
  w.part = w.rec_dvl + (size_t)NB_DVL_REC * N->n_dvl;
  return w;
}

// error partials of every factor kind into part[0 .. n_imu + n_dvl + n_diag), reduced into out[0]; mode 0 also writes
// the IMU / DVL records and accumulates the diagonal factors into (Snav, gnav)
int navb_errors(const vus_navb_factors* N, const double* poses, const double* vels, const double* biases,
                const double* dc, int mode, const NavbWork& w, double* Snav, double* gnav, double* out, hipStream_t st) {
  const int n_diag = N->n_vprior + N->n_bbetween + N->n_bprior;
  if (N->n_imu > 0)
    navb_imu_kernel<<<cdivb(N->n_imu, 64), 64, 0, st>>>(*N, poses, vels, biases, dc, w.rec_imu, w.part, mode);
  if (N->n_dvl > 0)
    navb_dvl_kernel<<<cdivb(N->n_dvl, 64), 64, 0, st>>>(*N, poses, vels, dc, w.rec_dvl, w.part + N->n_imu, mode);
  if (n_diag > 0)
    navb_diag_kernel<<<cdivb(n_diag, 64), 64, 0, st>>>(*N, vels, biases, dc, Snav, gnav, w.part + N->n_imu + N->n_dvl, mode);
  navb_reduce_kernel<<<1, 1024, 0, st>>>(w.part, N->n_imu + N->n_dvl + n_diag, out);
  VUS_CHECK_LAUNCH("navb_errors");
  return VUS_OK;
}

}  // namespace

// work layout: [records of the IMU factors | records of the DVL factors | error partials]
extern "C" long long vus_navb_work_doubles(const vus_navb_factors* N) {
  if (!N) return 0;
  return (long long)NB_IMU_REC * N->n_imu + (long long)NB_DVL_REC * N->n_dvl + N->n_imu + N->n_dvl + N->n_vprior +
         N->n_bbetween + N->n_bprior + 8;
}

extern "C" int vus_navb_linearize(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                                  const double* biases, double* Snav, double* gnav, double* err, double* work,
                                  void* stream) {
  VUS_REQUIRE(poses && vels && biases && Snav && gnav && err && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  hipStream_t st = vus::as_stream(stream);
  const size_t n_nodes = 3 * (size_t)n_poses;
  VUS_CHECK_HIP(hipMemsetAsync(Snav, 0, sizeof(double) * 36 * NB_SDIAG * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(gnav, 0, sizeof(double) * 6 * n_nodes, st));
  const NavbWork w = split_work(N, work);
  if (int rc = navb_errors(N, poses, vels, biases, nullptr, 0, w, Snav, gnav, err, st)) return rc;
  if (N->n_imu > 0) navb_accumulate_imu_kernel<<<N->n_imu, 640, 0, st>>>(*N, w.rec_imu, Snav, gnav);
  if (N->n_dvl > 0) navb_accumulate_dvl_kernel<<<N->n_dvl, 128, 0, st>>>(*N, w.rec_dvl, Snav, gnav);
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
  navb_assemble_kernel<<<cdivb(36ll * n_nodes, 256), 256, 0, vus::as_stream(stream)>>>(n_nodes, band, lambda, Snav, gnav,
                                                                                     Sband, gs);
  VUS_CHECK_LAUNCH("navb_assemble");
  return VUS_OK;
}

extern "C" int vus_navb_eval_step(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                                  const double* biases, const double* dc, const double* new_poses, double* new_vels,
                                  double* new_biases, double* out, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && dc && new_poses && new_vels && new_biases && out && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  hipStream_t st = vus::as_stream(stream);
  navb_retract_kernel<<<cdivb(6ll * n_poses, 256), 256, 0, st>>>(n_poses, vels, biases, dc, new_vels, new_biases);
  const NavbWork w = split_work(N, work);
  if (int rc = navb_errors(N, poses, vels, biases, dc, 2, w, nullptr, nullptr, out, st)) return rc;
  return navb_errors(N, new_poses, new_vels, new_biases, nullptr, 1, w, nullptr, nullptr, out + 1, st);
}

extern "C" int vus_navb_error(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                              const double* biases, double* err, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && err && work, "null buffer");
  if (int rc = check_navb(N, n_poses)) return rc;
  return navb_errors(N, poses, vels, biases, nullptr, 1, split_work(N, work), nullptr, nullptr, err,
                     vus::as_stream(stream));
}
