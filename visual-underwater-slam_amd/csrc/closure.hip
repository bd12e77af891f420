// closure.hip -- long loop closures as a low-rank term of the reduced camera system, gfx950 (MI355X), fp64
// (include/vus_closure.h).  A between factor further apart than the band is not added to Sband: its whitened Jacobian rows
// are kept, S = B + U U^T, and every solution of the band system B is corrected by x <- x - Z C^-1 (U^T x), Z = B^-1 U from
// vus_ba_band_resolve (band_resolve.hip), C = I + U^T Z.
//   linearize    thread / factor    the factor's rows [J1 J2 r], whitened and reweighted (between_device.h: the arithmetic
//                                   of the in-band path), its error to a partial
//   gradient     6 threads          gs += J^T r at both nodes, thread = tangent component, factors in order
//   scatter      thread / element   the rows into U, one right-hand side per Jacobian row
//   cap_entries  thread / entry     C = I + U^T Z, a 12-term dot product each
//   cap_chol     one workgroup      left-looking Cholesky of C in place: thread = row, one column per step
//   solve        workgroup / rhs    v = U^T x, C w = v by substitution with the factor
//   apply        thread / row       x -= Z w
// Every sum has a fixed order and nothing is atomic: two runs give the same bits.
#include <cmath>
#include <cstdlib>
#include <vector>
#include "vus_common.h"
#include "se3_device.h"
#include "between_device.h"
#include "factor_common.h"
#include "../../include/vus_closure.h"

namespace {

constexpr int ROW = VUS_CLOSURE_ROW;                 // J1 (36), J2 (36), r (6)
constexpr int MAX_M = 6 * VUS_CLOSURE_MAX;           // columns of U

// FULL: the factors carry a full-covariance model (B.sqrt_info); the diagonal instantiation is the kernel as it was.
template <bool FULL>
__global__ __launch_bounds__(64) void closure_linearize_kernel(vus_between_factors B, const double* __restrict__ poses,
                                                               double* __restrict__ rows, double* __restrict__ err_part) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= B.n) return;
  BetweenLin L;
  between_factor<true>(B, poses, f, L);
  if constexpr (FULL) {
    // sw R H1, sw R (upper-triangular, the zeros written), sw R r: the whitening of the in-band path (between_device.h)
    SqrtInfo S;
    load_sqrt_info(B, f, S);
    double b[6], rw, rho;
    whiten6(S, 1.0, L.r, b);
    const double d2 = norm_sq6(b);
    robust_weight_of(B.loss_kind, B.loss_k, f, d2, rw, rho);
    const double sw = sqrt(rw);
    double* o = rows + ROW * (size_t)f;
    whiten66(S, sw, L.H1, o);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
      for (int c = 0; c < 6; ++c) o[36 + 6 * q + c] = c >= q ? S.R[SqrtInfo::at(q, c >= q ? c : q)] * sw : 0.0;
      o[72 + q] = b[q] * sw;
    }
    err_part[f] = 0.5 * rw * d2;
    return;
  }
  double w[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = B.w[6 * (size_t)f + k];
  double rw, rho;
  const double d2 = whitened_sq(w, L.r);
  robust_weight_of(B.loss_kind, B.loss_k, f, d2, rw, rho);
  const double sw = sqrt(rw);
  double* o = rows + ROW * (size_t)f;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double s = sw * w[q];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      o[6 * q + c] = s * L.H1[6 * q + c];
      o[36 + 6 * q + c] = q == c ? s : 0.0;
    }
    o[72 + q] = s * L.r[q];
  }
  err_part[f] = 0.5 * rw * d2;
}

// a node of the set as the kernels use it: inside the problem (vus_closure_check refuses anything else)
__device__ __forceinline__ bool node_ok(const vus_between_factors& B, int node) { return (unsigned)node < (unsigned)B.n_nodes; }

__global__ __launch_bounds__(64) void closure_gradient_kernel(vus_between_factors B, const double* __restrict__ rows,
                                                              double* __restrict__ gs) {
  const int c = threadIdx.x;
  if (c >= 6) return;
  for (int f = 0; f < B.n; ++f) {
    const double* o = rows + ROW * (size_t)f;
    const int n1 = B.node1[f], n2 = B.node2[f];
    if (!node_ok(B, n1) || !node_ok(B, n2)) continue;
    double g1 = 0, g2 = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      g1 += o[6 * q + c] * o[72 + q];
      g2 += o[36 + 6 * q + c] * o[72 + q];
    }
    gs[6 * (size_t)n1 + c] += g1;
    gs[6 * (size_t)n2 + c] += g2;
  }
}

__global__ __launch_bounds__(256) void closure_scatter_kernel(vus_between_factors B, const double* __restrict__ rows,
                                                              double* __restrict__ U) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 72 * B.n) return;
  const int f = t / 72, e = t - 72 * f;
  const int half = e / 36, q = (e - 36 * half) / 6, c = e % 6;
  const int node = half ? B.node2[f] : B.node1[f];
  if (!node_ok(B, node)) return;
  U[(size_t)(6 * f + q) * (6 * (size_t)B.n_nodes) + 6 * (size_t)node + c] = rows[ROW * (size_t)f + e];
}

// column a of U against a vector x over the nodes: the 12 terms of factor a / 6, row a % 6
__device__ __forceinline__ double u_dot(const vus_between_factors& B, const double* __restrict__ rows, int a,
                                        const double* __restrict__ x) {
  const int f = a / 6, q = a - 6 * f;
  const double* o = rows + ROW * (size_t)f;
  const int n1 = B.node1[f], n2 = B.node2[f];
  if (!node_ok(B, n1) || !node_ok(B, n2)) return 0.0;
  double s = 0;
#pragma unroll
  for (int c = 0; c < 6; ++c) s += o[6 * q + c] * x[6 * (size_t)n1 + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) s += o[36 + 6 * q + c] * x[6 * (size_t)n2 + c];
  return s;
}

__global__ __launch_bounds__(256) void closure_cap_entries_kernel(vus_between_factors B, const double* __restrict__ rows,
                                                                  const double* __restrict__ Z, double* __restrict__ C) {
  const int m = 6 * B.n;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * m) return;
  const int a = t / m, b = t - m * a;
  C[t] = (a == b ? 1.0 : 0.0) + u_dot(B, rows, a, Z + (size_t)b * (6 * (size_t)B.n_nodes));
}

// thread = row i.  Column j: s_i = C_ij - sum_{c < j} C_ic C_jc (the columns before j are final), then the pivot's root.
// The products are summed first and taken from C_ij once: C is I plus a term that is small for weak closures, and a running
// difference would round at the size of C_ij in each of up to 383 steps (12 x LAPACK's residual at m = 384 on the MI355X).
__global__ __launch_bounds__(MAX_M) void closure_cap_chol_kernel(int m, double* C) {
  const int i = threadIdx.x;
  __shared__ double piv;
  for (int j = 0; j < m; ++j) {
    double s = 0.0;
    if (i >= j && i < m) {
      double dot = 0.0;
      for (int c = 0; c < j; ++c) dot += C[i * m + c] * C[j * m + c];
      s = C[i * m + j] - dot;
    }
    if (i == j) piv = sqrt(s);
    __syncthreads();
    if (i >= j && i < m) C[i * m + j] = i == j ? piv : s / piv;
    __syncthreads();
  }
}

// thread = row i of the factor: C_ii = sum_{c <= i} L_ic^2, then the largest over the rows (a NaN row wins)
__global__ __launch_bounds__(MAX_M) void closure_diag_max_kernel(int m, const double* __restrict__ C, double* __restrict__ out) {
  const int i = threadIdx.x;
  __shared__ double v[MAX_M];
  double s = 0.0;
  if (i < m)
    for (int c = 0; c <= i; ++c) s += C[i * m + c] * C[i * m + c];
  v[i] = s;
  __syncthreads();
  if (i == 0) {
    double best = v[0];
    for (int a = 1; a < m; ++a) best = (v[a] > best || v[a] != v[a]) ? v[a] : best;
    out[0] = best;
  }
}

// block = right-hand side: w = C^-1 (U^T x) -> W [n_rhs, m]
__global__ __launch_bounds__(MAX_M) void closure_solve_kernel(vus_between_factors B, const double* __restrict__ rows,
                                                              const double* __restrict__ C, const double* __restrict__ X,
                                                              double* __restrict__ W) {
  const int m = 6 * B.n, a = threadIdx.x;
  const double* x = X + (size_t)blockIdx.x * (6 * (size_t)B.n_nodes);
  __shared__ double v[MAX_M];
  if (a < m) v[a] = u_dot(B, rows, a, x);
  __syncthreads();
  for (int j = 0; j < m; ++j) {                 // L y = v
    if (a == j) v[j] /= C[j * m + j];
    __syncthreads();
    if (a > j && a < m) v[a] -= C[a * m + j] * v[j];
    __syncthreads();
  }
  for (int j = m - 1; j >= 0; --j) {            // L^T w = y
    if (a == j) v[j] /= C[j * m + j];
    __syncthreads();
    if (a < j) v[a] -= C[j * m + a] * v[j];
    __syncthreads();
  }
  if (a < m) W[(size_t)blockIdx.x * m + a] = v[a];
}

// x[row] -= sum_a Z[a][row] w[a]; blockIdx.y = right-hand side
__global__ __launch_bounds__(256) void closure_apply_kernel(int m, size_t ld, const double* __restrict__ Z,
                                                            const double* __restrict__ W, double* __restrict__ X) {
  __shared__ double w[MAX_M];
  for (int a = threadIdx.x; a < m; a += blockDim.x) w[a] = W[(size_t)blockIdx.y * m + a];
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= ld) return;
  double s = 0.0;
  for (int a = 0; a < m; ++a) s += Z[(size_t)a * ld + row] * w[a];
  X[(size_t)blockIdx.y * ld + row] -= s;
}

int check_args(const vus_between_factors* B) {
  VUS_REQUIRE(B != nullptr, "closure factors are null");
  VUS_REQUIRE(B->n >= 1 && B->n <= VUS_CLOSURE_MAX, "n=%d long closures, [1, %d] are supported", B->n, VUS_CLOSURE_MAX);
  VUS_REQUIRE(B->n_nodes >= 2 && B->pose_stride >= 1 && B->pose_stride <= 3 && B->n_nodes % B->pose_stride == 0,
              "bad sizes: n_nodes=%d pose_stride=%d", B->n_nodes, B->pose_stride);
  VUS_REQUIRE(B->node1 && B->node2 && B->meas && (B->w || B->sqrt_info) && B->loss_kind && B->loss_k, "factor arrays are null");
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_closure_work_doubles(const vus_between_factors* B) {
  if (!B || B->n < 0) return 0;
  return 6ll * VUS_CLOSURE_MAX_RHS * B->n + 8;      // correct: n_rhs x 6 n; also the 2 n + 8 of vus_between_eval_step
}

extern "C" int vus_closure_check(const vus_between_factors* B, int band, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(band >= 0 && band < B->n_nodes, "band=%d for %d nodes", band, B->n_nodes);
  hipStream_t st = vus::as_stream(stream);
  std::vector<int> n1, n2, kind;
  std::vector<double> lk;
  if (int rc = read_back(B->node1, B->n, n1, st)) return rc;
  if (int rc = read_back(B->node2, B->n, n2, st)) return rc;
  if (int rc = read_back(B->loss_kind, B->n, kind, st)) return rc;
  if (int rc = read_back(B->loss_k, B->n, lk, st)) return rc;
  const int ps = B->pose_stride;
  for (int f = 0; f < B->n; ++f) {
    VUS_REQUIRE(n1[f] >= 0 && n1[f] < B->n_nodes && n2[f] >= 0 && n2[f] < B->n_nodes && n1[f] % ps == 0 && n2[f] % ps == 0,
                "factor %d: nodes (%d, %d) are not pose nodes of %d nodes at pose_stride %d", f, n1[f], n2[f], B->n_nodes, ps);
    VUS_REQUIRE(std::abs(n1[f] - n2[f]) > band, "factor %d: nodes %d and %d are inside the band of %d nodes: it belongs to the "
                "in-band between factors", f, n1[f], n2[f], band);
    if (int rc = check_factor_loss(f, kind[f], lk[f])) return rc;
  }
  return check_sqrt_info(B->sqrt_info, B->n, st);
}

extern "C" int vus_closure_linearize(const vus_between_factors* B, const double* poses, double* rows, double* err,
                                     double* work, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(poses && rows && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (B->sqrt_info) closure_linearize_kernel<true><<<cdiv(B->n, 64), 64, 0, st>>>(*B, poses, rows, work);
  else closure_linearize_kernel<false><<<cdiv(B->n, 64), 64, 0, st>>>(*B, poses, rows, work);
  vus::reduce_partials(work, B->n, err, st);
  VUS_CHECK_LAUNCH("closure_linearize");
  return VUS_OK;
}

extern "C" int vus_closure_gradient(const vus_between_factors* B, const double* rows, double* gs, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(rows && gs, "null buffer");
  closure_gradient_kernel<<<1, 64, 0, vus::as_stream(stream)>>>(*B, rows, gs);
  VUS_CHECK_LAUNCH("closure_gradient");
  return VUS_OK;
}

extern "C" int vus_closure_scatter(const vus_between_factors* B, const double* rows, double* U, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(rows && U, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  VUS_CHECK_HIP(hipMemsetAsync(U, 0, sizeof(double) * 36 * (size_t)B->n * (size_t)B->n_nodes, st));
  closure_scatter_kernel<<<cdiv(72ll * B->n, 256), 256, 0, st>>>(*B, rows, U);
  VUS_CHECK_LAUNCH("closure_scatter");
  return VUS_OK;
}

extern "C" int vus_closure_capacitance(const vus_between_factors* B, const double* rows, const double* Z, double* C,
                                       void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(rows && Z && C, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  const int m = 6 * B->n;
  closure_cap_entries_kernel<<<cdiv((long long)m * m, 256), 256, 0, st>>>(*B, rows, Z, C);
  VUS_CHECK_LAUNCH("closure_capacitance entries");
  closure_cap_chol_kernel<<<1, MAX_M, 0, st>>>(m, C);
  VUS_CHECK_LAUNCH("closure_capacitance factor");
  return VUS_OK;
}

extern "C" int vus_closure_diag_max(const vus_between_factors* B, const double* C, double* out, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(C && out, "null buffer");
  closure_diag_max_kernel<<<1, MAX_M, 0, vus::as_stream(stream)>>>(6 * B->n, C, out);
  VUS_CHECK_LAUNCH("closure_diag_max");
  return VUS_OK;
}

extern "C" int vus_closure_correct(const vus_between_factors* B, const double* rows, const double* Z, const double* C,
                                   double* X, int n_rhs, double* work, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(rows && Z && C && X && work, "null buffer");
  VUS_REQUIRE(n_rhs >= 1 && n_rhs <= VUS_CLOSURE_MAX_RHS, "n_rhs=%d out of range [1, %d]", n_rhs, VUS_CLOSURE_MAX_RHS);
  hipStream_t st = vus::as_stream(stream);
  const int m = 6 * B->n;
  const size_t ld = 6 * (size_t)B->n_nodes;
  closure_solve_kernel<<<n_rhs, MAX_M, 0, st>>>(*B, rows, C, X, work);
  VUS_CHECK_LAUNCH("closure_correct solve");
  closure_apply_kernel<<<dim3(cdiv((long long)ld, 256), n_rhs), 256, 0, st>>>(m, ld, Z, work, X);
  VUS_CHECK_LAUNCH("closure_correct apply");
  return VUS_OK;
}
