// combined_imu.hip -- gtsam.CombinedImuFactor for gfx950 (MI355X), fp64, in the per-keyframe-bias layout
// (include/vus_combined_imu.h, family `cimu`): one 15-row factor on X_i, V_i, X_j, V_j, B_i, B_j (j = i + 1) whitened with
// the full 15 x 15 covariance of the preintegrated measurement and the bias walk.  Rows 0..8 are imu_factor of
// imu_device.h, the copy nav.hip uses; rows 9..14 are b_j - b_i.
//   cimu_linearize   workgroup / factor.  Thread 0 evaluates imu_factor (its 9 x 24 Jacobian is 216 doubles of scratch, as
//                    in nav.hip's one-thread-per-factor kernel) and leaves r and J in LDS; 465 threads then form one entry
//                    each of the whitened [Jw | rw] = W [J | r] (15 x 31) in LDS -- the 15 x 30 whitened Jacobian never
//                    exists in one thread's registers or scratch -- and the 900 entries of Jw^T Jw and 30 of Jw^T rw are
//                    dealt over the workgroup and added to their blocks with f64 atomics, as nav_accumulate_imu_kernel
//                    does for 24 x 24.  Thread 0 writes the factor's error partial.
//   cimu_eval        thread / factor: the error (mode 1) or the linearised error at the node step (mode 2).  W (r + J d)
//                    needs the unwhitened 9 x 24 Jacobian only: u = r + J d is 15 numbers, whitened row by row.
//   cimu_assemble    thread / element of a node's 6 x 6 blocks: Sband += Scimu on 6 diagonals, gs += gcimu (one owner each)
// Launches only: no workgroup waits for another.  Errors are reduced in index order (vus::reduce_partials).
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "imu_device.h"
#include "factor_common.h"
#include "../../include/vus_combined_imu.h"

namespace {

constexpr int CI_ROWS = 15, CI_COLS = 30, CI_LD = 31;   // [Jw | rw]: 30 Jacobian columns and the residual
constexpr int CI_SDIAG = 6;                             // block diagonals of Scimu
constexpr int CI_WG = 256;

// column c of the 15 x 30 Jacobian -> (node, dim): X_i V_i X_j V_j B_i B_j with j = i + 1 (checked on the host)
__device__ __forceinline__ void cimu_col(int c, int i, int& node, int& dim) {
  if (c < 6) { node = 3 * i; dim = c; }
  else if (c < 9) { node = 3 * i + 1; dim = c - 6; }
  else if (c < 15) { node = 3 * i + 3; dim = c - 9; }
  else if (c < 18) { node = 3 * i + 4; dim = c - 15; }
  else if (c < 24) { node = 3 * i + 2; dim = c - 18; }
  else { node = 3 * i + 5; dim = c - 24; }
}

// entry (k, c) of the unwhitened [J | r] (15 x 31) from the ImuFactor's J9 [9][24], r9 [9] and the bias difference db [6]
__device__ __forceinline__ double cimu_unwhitened(const double* J9, const double* r9, const double* db, int k, int c) {
  if (k < 9) return c < 24 ? J9[24 * k + c] : (c < 30 ? 0.0 : r9[k]);
  const int b = k - 9;
  if (c == 30) return db[b];
  return c == 18 + b ? -1.0 : (c == 24 + b ? 1.0 : 0.0);
}

__global__ __launch_bounds__(CI_WG) void cimu_linearize_kernel(vus_cimu_factors F, const double* __restrict__ poses,
                                                               const double* __restrict__ vels,
                                                               const double* __restrict__ biases, double* __restrict__ Scimu,
                                                               double* __restrict__ gcimu, double* __restrict__ part) {
  __shared__ double s_J[9 * 24], s_r[9], s_db[6], s_W[CI_ROWS * CI_ROWS], s_Jw[CI_ROWS * CI_LD];
  const int t = threadIdx.x, f = blockIdx.x;
  const int i = F.i[f], j = i + 1;
  for (int k = t; k < CI_ROWS * CI_ROWS; k += CI_WG) s_W[k] = F.W[CI_ROWS * CI_ROWS * (size_t)f + k];
  if (t == 0) {
    double r[9], J[9 * 24];
    imu_factor(poses + 12 * (size_t)i, vels + 3 * (size_t)i, poses + 12 * (size_t)j, vels + 3 * (size_t)j,
               biases + 6 * (size_t)i, F.pim + PIM_N * (size_t)f, F.gravity, r, J);
    for (int k = 0; k < 9 * 24; ++k) s_J[k] = J[k];
    for (int k = 0; k < 9; ++k) s_r[k] = r[k];
    for (int k = 0; k < 6; ++k) s_db[k] = biases[6 * (size_t)j + k] - biases[6 * (size_t)i + k];
  }
  __syncthreads();
  for (int e = t; e < CI_ROWS * CI_LD; e += CI_WG) {     // [Jw | rw] = W [J | r]
    const int a = e / CI_LD, c = e - CI_LD * a;
    double v = 0.0;
    for (int k = 0; k < CI_ROWS; ++k) v += s_W[CI_ROWS * a + k] * cimu_unwhitened(s_J, s_r, s_db, k, c);
    s_Jw[e] = v;
  }
  __syncthreads();
  for (int e = t; e < CI_COLS * CI_LD; e += CI_WG) {     // (c1, c2 < 30): Jw^T Jw;  (c1, 30): the gradient Jw^T rw
    const int c1 = e / CI_LD, c2 = e - CI_LD * c1;
    int n1, d1, n2 = 0, d2 = 0;
    cimu_col(c1, i, n1, d1);
    if (c2 < CI_COLS) {
      cimu_col(c2, i, n2, d2);
      if (n1 < n2) continue;                             // the upper triangle is the transpose of what the lower one stores
    }
    double h = 0.0;
#pragma unroll
    for (int a = 0; a < CI_ROWS; ++a) h += s_Jw[CI_LD * a + c1] * s_Jw[CI_LD * a + c2];
    if (c2 < CI_COLS) unsafeAtomicAdd(&Scimu[36 * ((size_t)n1 * CI_SDIAG + (n1 - n2)) + 6 * d1 + d2], h);
    else unsafeAtomicAdd(&gcimu[6 * (size_t)n1 + d1], h);
  }
  if (t == 0) {
    double e = 0.0;
    for (int a = 0; a < CI_ROWS; ++a) e += 0.5 * s_Jw[CI_LD * a + CI_COLS] * s_Jw[CI_LD * a + CI_COLS];
    part[f] = e;
  }
}

// mode 1: error only;  mode 2: linearised error 0.5 |W (r + J d)|^2 with d from the node step dc
__global__ void cimu_eval_kernel(vus_cimu_factors F, const double* __restrict__ poses, const double* __restrict__ vels,
                                 const double* __restrict__ biases, const double* __restrict__ dc, double* __restrict__ part,
                                 int mode) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F.n) return;
  const int i = F.i[f], j = i + 1;
  double u[CI_ROWS], J[9 * 24];
  imu_factor(poses + 12 * (size_t)i, vels + 3 * (size_t)i, poses + 12 * (size_t)j, vels + 3 * (size_t)j,
             biases + 6 * (size_t)i, F.pim + PIM_N * (size_t)f, F.gravity, u, mode == 2 ? J : nullptr);
  for (int k = 0; k < 6; ++k) u[9 + k] = biases[6 * (size_t)j + k] - biases[6 * (size_t)i + k];
  if (mode == 2) {
    for (int c = 0; c < 24; ++c) {
      int node, dim;
      cimu_col(c, i, node, dim);
      const double d = dc[6 * (size_t)node + dim];
      for (int k = 0; k < 9; ++k) u[k] += J[24 * k + c] * d;
    }
    for (int k = 0; k < 6; ++k) u[9 + k] += dc[6 * (size_t)(3 * i + 5) + k] - dc[6 * (size_t)(3 * i + 2) + k];
  }
  const double* W = F.W + CI_ROWS * CI_ROWS * (size_t)f;
  double e = 0.0;
  for (int a = 0; a < CI_ROWS; ++a) {
    double rw = 0.0;
    for (int k = 0; k < CI_ROWS; ++k) rw += W[CI_ROWS * a + k] * u[k];
    e += 0.5 * rw * rw;
  }
  part[f] = e;
}

__global__ void cimu_assemble_kernel(int n_nodes, int band, const double* __restrict__ Scimu, const double* __restrict__ gcimu,
                                     double* __restrict__ Sband, double* __restrict__ gs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * n_nodes) return;
  const int node = t / 36, e = t - 36 * node;
  const int smax = min(CI_SDIAG - 1, min(band, node));
  for (int s = 0; s <= smax; ++s) Sband[36 * ((size_t)node * (band + 1) + s) + e] += Scimu[36 * ((size_t)node * CI_SDIAG + s) + e];
  if (e < 6) gs[6 * (size_t)node + e] += gcimu[6 * (size_t)node + e];
}

// every size, pointer and index the kernels rely on, checked on the host before anything is launched
int check_cimu(const vus_cimu_factors* F, int n_poses, hipStream_t st) {
  VUS_REQUIRE(F != nullptr, "combined IMU factors are null");
  VUS_REQUIRE(F->n >= 1, "combined IMU factors: n=%d must be >= 1", F->n);
  VUS_REQUIRE(n_poses >= 2, "combined IMU factors: n_poses=%d must be >= 2", n_poses);
  VUS_REQUIRE(F->i && F->j && F->pim && F->W, "combined IMU factor arrays are null");
  std::vector<int> a, b;
  if (int rc = read_back(F->i, (size_t)F->n, a, st)) return rc;
  if (int rc = read_back(F->j, (size_t)F->n, b, st)) return rc;
  for (int f = 0; f < F->n; ++f)
    VUS_REQUIRE(a[f] >= 0 && a[f] + 1 < n_poses && b[f] == a[f] + 1,
                "CombinedImuFactor %d joins keyframes %d and %d: needs j = i + 1 < n_poses=%d", f, a[f], b[f], n_poses);
  return VUS_OK;
}

int cimu_errors(const vus_cimu_factors* F, const double* poses, const double* vels, const double* biases, const double* dc,
                int mode, double* out, double* work, hipStream_t st) {
  cimu_eval_kernel<<<cdiv(F->n, 64), 64, 0, st>>>(*F, poses, vels, biases, dc, work, mode);
  vus::reduce_partials(work, F->n, out, st);
  VUS_CHECK_LAUNCH("cimu_errors");
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_cimu_work_doubles(const vus_cimu_factors* F) {
  if (!F || F->n < 1) return 0;
  return (long long)F->n + 8;
}

extern "C" int vus_cimu_linearize(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels,
                                  const double* biases, double* Scimu, double* gcimu, double* err, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && Scimu && gcimu && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (int rc = check_cimu(F, n_poses, st)) return rc;
  const size_t n_nodes = 3 * (size_t)n_poses;
  VUS_CHECK_HIP(hipMemsetAsync(Scimu, 0, sizeof(double) * 36 * CI_SDIAG * n_nodes, st));
  VUS_CHECK_HIP(hipMemsetAsync(gcimu, 0, sizeof(double) * 6 * n_nodes, st));
  cimu_linearize_kernel<<<F->n, CI_WG, 0, st>>>(*F, poses, vels, biases, Scimu, gcimu, work);
  vus::reduce_partials(work, F->n, err, st);
  VUS_CHECK_LAUNCH("cimu_linearize");
  return VUS_OK;
}

extern "C" int vus_cimu_assemble(int n_nodes, int band, const double* Scimu, const double* gcimu, double* Sband, double* gs,
                                 void* stream) {
  VUS_REQUIRE(Scimu && gcimu && Sband && gs, "null buffer");
  VUS_REQUIRE(n_nodes >= 6 && n_nodes % 3 == 0, "n_nodes=%d is not 3 * n_poses with n_poses >= 2", n_nodes);
  VUS_REQUIRE(band >= (n_nodes - 1 < 5 ? n_nodes - 1 : 5) && band < n_nodes, "band=%d for %d nodes: a CombinedImuFactor needs "
              "min(5, n_nodes - 1) <= band < n_nodes", band, n_nodes);
  cimu_assemble_kernel<<<cdiv(36ll * n_nodes, 256), 256, 0, vus::as_stream(stream)>>>(n_nodes, band, Scimu, gcimu, Sband, gs);
  VUS_CHECK_LAUNCH("cimu_assemble");
  return VUS_OK;
}

extern "C" int vus_cimu_eval_step(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels,
                                  const double* biases, const double* dc, const double* new_poses, const double* new_vels,
                                  const double* new_biases, double* out, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && dc && new_poses && new_vels && new_biases && out && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (int rc = check_cimu(F, n_poses, st)) return rc;
  if (int rc = cimu_errors(F, poses, vels, biases, dc, 2, out, work, st)) return rc;
  return cimu_errors(F, new_poses, new_vels, new_biases, nullptr, 1, out + 1, work, st);
}

extern "C" int vus_cimu_error(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels,
                              const double* biases, double* err, double* work, void* stream) {
  VUS_REQUIRE(poses && vels && biases && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (int rc = check_cimu(F, n_poses, st)) return rc;
  return cimu_errors(F, poses, vels, biases, nullptr, 1, err, work, st);
}
