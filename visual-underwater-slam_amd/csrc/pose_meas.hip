// pose_meas.hip -- position and attitude fixes on keyframe poses for gfx950 (MI355X), fp64 (include/vus_pose_meas.h).
//
// A unary 3-row factor on a pose adds to the pose's information block Hpp and gradient gp between the linearisation of the
// observations and the landmark Schur step; nothing downstream of Hpp / gp knows of it.
//   linearize   thread / factor-carrying pose (a CSR row): the 21 + 6 sums of J^T J and J^T r of its factors in CSR order
//               in registers, then Hpp[i], gp[i] += them with plain loads and stores (a row owns its pose: no atomics);
//               the row's error to the workgroup's partial
//   eval        thread / row: the linearised error at the step (old poses) and the error at new_poses (or at poses alone
//               for vus_pose_meas_error)
//   weights     thread / row: w(d) of its factors
// Errors: a fixed LDS tree per workgroup -> one partial per workgroup in `work` -> vus::reduce_partials in index order.
// Shared with the other pose kernels (se3_device.h): so3_logmap, load12, the robust-loss table and its per-factor dispatcher;
// with point_prior.hip (factor_common.h): that tree (block_partial), the guarded row lookup (csr_row), and on the host
// read_back, zero_out and the row, weight and loss checks.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "se3_device.h"
#include "factor_common.h"

namespace {

constexpr int WG = 256;       // 4 waves of 64; one row per thread

// factor f at the pose T (flat12): the unwhitened residual r [3], the whitening w [3], d2 = |W r|^2 and, WITH_J, the
// unwhitened Jacobian J [3][6] in the tangent order (omega, v)
template <bool WITH_J>
__device__ __forceinline__ void factor_at(const vus_pose_meas& M, int f, const double* T, double* r, double* w, double& d2,
                                          double (*J)[6]) {
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = M.meas[9 * (size_t)f + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = M.w[3 * (size_t)f + k];
  if (M.kind[f] == VUS_POSE_MEAS_ROTATION) {
    double E[9];                                          // Rm^T R
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) E[3 * a + c] = m[a] * T[c] + m[3 + a] * T[3 + c] + m[6 + a] * T[6 + c];
    so3_logmap(E, r);
    if (WITH_J) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) J[a][c] = a == c ? 1.0 : 0.0;
    }
  } else {                                                // r = t + R a - m,  J = [ -R [a]x , R ]
    const double* la = m + 3;
    const double ax[9] = {0, -la[2], la[1], la[2], 0, -la[0], -la[1], la[0], 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = (T[9 + a] - m[a]) + (T[3 * a] * la[0] + T[3 * a + 1] * la[1] + T[3 * a + 2] * la[2]);
      if (WITH_J) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          J[a][c] = -(T[3 * a] * ax[c] + T[3 * a + 1] * ax[3 + c] + T[3 * a + 2] * ax[6 + c]);
          J[a][3 + c] = T[3 * a + c];
        }
      }
    }
  }
  d2 = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) d2 += (w[k] * r[k]) * (w[k] * r[k]);
}

// slot of (a, c), a <= c, in the packed upper triangle of a 6 x 6 block
__device__ __host__ constexpr int tri(int a, int c) { return 6 * a - a * (a - 1) / 2 + (c - a); }

__global__ __launch_bounds__(WG) void pose_meas_linearize_kernel(vus_pose_meas M, const double* __restrict__ poses,
                                                                 double* __restrict__ Hpp, double* __restrict__ gp,
                                                                 double* __restrict__ err_part) {
  const int row = blockIdx.x * WG + threadIdx.x;
  int i, a, b;
  double e = 0;
  if (csr_row(M.n_rows, M.row_pose, M.row_ptr, M.n_poses, M.n, row, i, a, b)) {
    double T[12];
    load12(poses + 12 * (size_t)i, T);
    double h[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) h[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
    for (int f = a; f < b; ++f) {
      double r[3], w[3], J[3][6], d2, rw, rho;
      factor_at<true>(M, f, T, r, w, d2, J);
      robust_weight_of(M.loss_kind, M.loss_k, f, d2, rw, rho);
      double w2[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) w2[k] = rw * w[k] * w[k];     // the weighted information of each residual row
#pragma unroll
      for (int x = 0; x < 6; ++x) {
#pragma unroll
        for (int y = x; y < 6; ++y) h[tri(x, y)] += J[0][x] * w2[0] * J[0][y] + J[1][x] * w2[1] * J[1][y] + J[2][x] * w2[2] * J[2][y];
        g[x] += J[0][x] * w2[0] * r[0] + J[1][x] * w2[1] * r[1] + J[2][x] * w2[2] * r[2];
      }
      e += 0.5 * rw * d2;
    }
    double* H = Hpp + 36 * (size_t)i;
    double* G = gp + 6 * (size_t)i;
#pragma unroll
    for (int x = 0; x < 6; ++x) {
#pragma unroll
      for (int y = 0; y < 6; ++y) H[6 * x + y] += h[x <= y ? tri(x, y) : tri(y, x)];
      G[x] += g[x];
    }
  }
  block_partial<WG>(e, err_part);
}

// part_lin[block] = the rows' 0.5 sum w |b + J d|^2 at the old poses with d = dp[pose_stride * i] (skipped when part_lin is
// null), part_new[block] = their sum rho at new_poses
__global__ __launch_bounds__(WG) void pose_meas_eval_kernel(vus_pose_meas M, const double* __restrict__ poses,
                                                            const double* __restrict__ dp,
                                                            const double* __restrict__ new_poses,
                                                            double* __restrict__ part_lin, double* __restrict__ part_new) {
  const int row = blockIdx.x * WG + threadIdx.x;
  int i, a, b;
  const bool has = csr_row(M.n_rows, M.row_pose, M.row_ptr, M.n_poses, M.n, row, i, a, b);
  // one pass per output over ONE instance of the factor code: pass 0 at the old poses with the step, pass 1 at new_poses
  double e_lin = 0, e_new = 0;
  if (has) {
#pragma nounroll
    for (int pass = part_lin != nullptr ? 0 : 1; pass < 2; ++pass) {
      double T[12], d[6];
      load12((pass ? new_poses : poses) + 12 * (size_t)i, T);
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = pass ? 0.0 : dp[6 * (size_t)M.pose_stride * i + k];
      double e = 0;
      for (int f = a; f < b; ++f) {
        double r[3], w[3], J[3][6], d2, rw, rho;
        factor_at<true>(M, f, T, r, w, d2, J);
        robust_weight_of(M.loss_kind, M.loss_k, f, d2, rw, rho);
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double v = r[k];
#pragma unroll
          for (int c = 0; c < 6; ++c) v += J[k][c] * d[c];
          s += (w[k] * v) * (w[k] * v);
        }
        e += pass ? rho : 0.5 * rw * s;
      }
      if (pass) e_new = e; else e_lin = e;
    }
  }
  if (part_lin != nullptr) {                              // uniform over the launch: the barriers stay convergent
    block_partial<WG>(e_lin, part_lin);
    __syncthreads();                                      // the LDS tree is reused below
  }
  block_partial<WG>(e_new, part_new);
}

__global__ __launch_bounds__(WG) void pose_meas_weights_kernel(vus_pose_meas M, const double* __restrict__ poses,
                                                               double* __restrict__ w_out) {
  const int row = blockIdx.x * WG + threadIdx.x;
  int i, a, b;
  if (!csr_row(M.n_rows, M.row_pose, M.row_ptr, M.n_poses, M.n, row, i, a, b)) return;
  double T[12];
  load12(poses + 12 * (size_t)i, T);
  for (int f = a; f < b; ++f) {
    double r[3], w[3], d2, rw, rho;
    factor_at<false>(M, f, T, r, w, d2, nullptr);
    robust_weight_of(M.loss_kind, M.loss_k, f, d2, rw, rho);
    w_out[f] = rw;
  }
}

int check_args(const vus_pose_meas* M) {
  VUS_REQUIRE(M != nullptr, "pose measurements are null");
  VUS_REQUIRE(M->n >= 0 && M->n_poses >= 0 && M->n_rows >= 0 && M->n_rows <= M->n && M->n_rows <= M->n_poses &&
                  (M->n == 0) == (M->n_rows == 0) && M->pose_stride >= 1 && M->pose_stride <= 3,
              "bad sizes: n=%d n_poses=%d n_rows=%d pose_stride=%d", M->n, M->n_poses, M->n_rows, M->pose_stride);
  VUS_REQUIRE(M->n == 0 || (M->row_pose && M->row_ptr && M->kind && M->meas && M->w && M->loss_kind && M->loss_k),
              "pose measurement arrays are null");
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_pose_meas_work_doubles(const vus_pose_meas* M) {
  if (!M || M->n_rows < 0) return 0;
  return 2ll * cdiv(M->n_rows, WG) + 8;
}

extern "C" int vus_pose_meas_check(const vus_pose_meas* M, void* stream) {
  if (int rc = check_args(M)) return rc;
  if (M->n == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const int n = M->n;
  std::vector<int> rp, ptr, kind, lkind;
  std::vector<double> meas, w, lk;
  if (int rc = read_back(M->row_pose, M->n_rows, rp, st)) return rc;
  if (int rc = read_back(M->row_ptr, (size_t)M->n_rows + 1, ptr, st)) return rc;
  if (int rc = read_back(M->kind, n, kind, st)) return rc;
  if (int rc = read_back(M->meas, 9 * (size_t)n, meas, st)) return rc;
  if (int rc = read_back(M->w, 3 * (size_t)n, w, st)) return rc;
  if (int rc = read_back(M->loss_kind, n, lkind, st)) return rc;
  if (int rc = read_back(M->loss_k, n, lk, st)) return rc;
  if (int rc = check_csr_rows(rp, ptr, M->n_rows, n, M->n_poses, "row_pose", "pose")) return rc;
  for (int f = 0; f < n; ++f) {
    VUS_REQUIRE(kind[f] == VUS_POSE_MEAS_POSITION || kind[f] == VUS_POSE_MEAS_ROTATION, "factor %d: unknown measurement kind %d",
                f, kind[f]);
    for (int k = 0; k < 3; ++k)
      if (int rc = check_factor_weight(f, w[3 * (size_t)f + k])) return rc;
    const double* m = meas.data() + 9 * (size_t)f;
    for (int k = 0; k < 9; ++k) VUS_REQUIRE(std::isfinite(m[k]), "factor %d: measurement %g is not finite", f, m[k]);
    if (kind[f] == VUS_POSE_MEAS_ROTATION) {
      double dev = 0;
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
          const double s = m[a] * m[c] + m[3 + a] * m[3 + c] + m[6 + a] * m[6 + c];
          dev = std::fmax(dev, std::fabs(s - (a == c ? 1.0 : 0.0)));
        }
      const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
      VUS_REQUIRE(dev <= 1e-9, "factor %d: the measured rotation is not orthonormal (max |R^T R - I| = %g)", f, dev);
      VUS_REQUIRE(det > 0.0, "factor %d: the measured rotation is a reflection (det = %g)", f, det);
    }
    if (int rc = check_factor_loss(f, lkind[f], lk[f])) return rc;
  }
  return VUS_OK;
}

extern "C" int vus_pose_meas_linearize(const vus_pose_meas* M, const double* poses, double* Hpp, double* gp, double* err,
                                       double* work, void* stream) {
  if (int rc = check_args(M)) return rc;
  VUS_REQUIRE(err != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (M->n == 0) return zero_out(err, 1, st);
  VUS_REQUIRE(poses && Hpp && gp && work, "null buffer");
  const int nb = cdiv(M->n_rows, WG);
  pose_meas_linearize_kernel<<<nb, WG, 0, st>>>(*M, poses, Hpp, gp, work);
  vus::reduce_partials(work, nb, err, st);
  VUS_CHECK_LAUNCH("pose_meas_linearize");
  return VUS_OK;
}

extern "C" int vus_pose_meas_eval_step(const vus_pose_meas* M, const double* poses, const double* dp,
                                       const double* new_poses, double* out, double* work, void* stream) {
  if (int rc = check_args(M)) return rc;
  VUS_REQUIRE(out != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (M->n == 0) return zero_out(out, 2, st);
  VUS_REQUIRE(poses && dp && new_poses && work, "null buffer");
  const int nb = cdiv(M->n_rows, WG);
  pose_meas_eval_kernel<<<nb, WG, 0, st>>>(*M, poses, dp, new_poses, work, work + nb);
  vus::reduce_partials(work, nb, out, st);
  vus::reduce_partials(work + nb, nb, out + 1, st);
  VUS_CHECK_LAUNCH("pose_meas_eval_step");
  return VUS_OK;
}

extern "C" int vus_pose_meas_error(const vus_pose_meas* M, const double* poses, double* err, double* work, void* stream) {
  if (int rc = check_args(M)) return rc;
  VUS_REQUIRE(err != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (M->n == 0) return zero_out(err, 1, st);
  VUS_REQUIRE(poses && work, "null buffer");
  const int nb = cdiv(M->n_rows, WG);
  pose_meas_eval_kernel<<<nb, WG, 0, st>>>(*M, nullptr, nullptr, poses, nullptr, work + nb);
  vus::reduce_partials(work + nb, nb, err, st);
  VUS_CHECK_LAUNCH("pose_meas_error");
  return VUS_OK;
}

extern "C" int vus_pose_meas_weights(const vus_pose_meas* M, const double* poses, double* w_out, void* stream) {
  if (int rc = check_args(M)) return rc;
  if (M->n == 0) return VUS_OK;
  VUS_REQUIRE(poses && w_out, "null buffer");
  pose_meas_weights_kernel<<<cdiv(M->n_rows, WG), WG, 0, vus::as_stream(stream)>>>(*M, poses, w_out);
  VUS_CHECK_LAUNCH("pose_meas_weights");
  return VUS_OK;
}
