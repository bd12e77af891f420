// point_prior.hip -- PriorFactor<Point3> kernels for gfx950 (MI355X), fp64 (include/vus_point_prior.h).
//
// A diagonal Gaussian prior on an observed landmark adds to the landmark's information block V and gradient gl between
// the linearisation of the observations and the landmark Schur step; nothing downstream of V / gl knows of it.
//   linearize   thread / prior-carrying landmark (a CSR row): V[j], gl[j] += its priors in CSR order, plain loads and
//               stores (a row owns its landmark: no atomics); the row's error to the workgroup's partial
//   eval        thread / row: the error at p + dl and at new_points (or at p alone for vus_point_prior_error)
// Errors: a fixed LDS tree per workgroup -> one partial per workgroup in `work` -> vus::reduce_partials in index order.
// Shared with pose_meas.hip (factor_common.h): that tree (block_partial), the guarded row lookup (csr_row), and on the host
// read_back, zero_out and the row and weight checks.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "factor_common.h"

namespace {

constexpr int WG = 256;       // 4 waves of 64; one row per thread

__device__ __forceinline__ void load3(const double* __restrict__ src, double* dst) {
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];      // [n,3] rows are 24 bytes: three double loads
}

// 0.5 sum |w (p - mean)|^2 over the factors [a, b)
__device__ __forceinline__ double row_error(const vus_point_priors& Q, int a, int b, const double* p) {
  double e = 0;
  for (int f = a; f < b; ++f) {
    double m[3], w[3];
    load3(Q.mean + 3 * (size_t)f, m);
    load3(Q.w + 3 * (size_t)f, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double t = w[k] * (p[k] - m[k]);
      e += t * t;
    }
  }
  return 0.5 * e;
}

__global__ __launch_bounds__(WG) void point_prior_linearize_kernel(vus_point_priors Q, const double* __restrict__ points,
                                                                   double* __restrict__ V, double* __restrict__ gl,
                                                                   double* __restrict__ err_part) {
  const int r = blockIdx.x * WG + threadIdx.x;
  int j, a, b;
  double e = 0;
  if (csr_row(Q.n_rows, Q.row_point, Q.row_ptr, Q.n_points, Q.n, r, j, a, b)) {
    double p[3], g[3];
    load3(points + 3 * (size_t)j, p);
    load3(gl + 3 * (size_t)j, g);
    double* Vj = V + 6 * (size_t)j;
    double h[3] = {Vj[0], Vj[3], Vj[5]};                  // xx, yy, zz of the upper triangle xx, xy, xz, yy, yz, zz
    for (int f = a; f < b; ++f) {
      double m[3], w[3];
      load3(Q.mean + 3 * (size_t)f, m);
      load3(Q.w + 3 * (size_t)f, w);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double w2 = w[k] * w[k], d = p[k] - m[k];
        h[k] += w2;
        g[k] += w2 * d;
        e += (w[k] * d) * (w[k] * d);
      }
    }
    Vj[0] = h[0]; Vj[3] = h[1]; Vj[5] = h[2];
    gl[3 * (size_t)j] = g[0]; gl[3 * (size_t)j + 1] = g[1]; gl[3 * (size_t)j + 2] = g[2];
    e *= 0.5;
  }
  block_partial<WG>(e, err_part);
}

// part_lin[block] = the rows' error at points + dl (skipped when part_lin is null), part_new[block] = at new_points
__global__ __launch_bounds__(WG) void point_prior_eval_kernel(vus_point_priors Q, const double* __restrict__ points,
                                                              const double* __restrict__ dl,
                                                              const double* __restrict__ new_points,
                                                              double* __restrict__ part_lin, double* __restrict__ part_new) {
  const int r = blockIdx.x * WG + threadIdx.x;
  int j, a, b;
  const bool has = csr_row(Q.n_rows, Q.row_point, Q.row_ptr, Q.n_points, Q.n, r, j, a, b);
  double p[3];
  if (part_lin != nullptr) {                              // uniform over the launch: the barriers below stay convergent
    double e = 0;
    if (has) {
      double d[3];
      load3(points + 3 * (size_t)j, p);
      load3(dl + 3 * (size_t)j, d);
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] += d[k];
      e = row_error(Q, a, b, p);
    }
    block_partial<WG>(e, part_lin);
    __syncthreads();                                      // the LDS tree is reused below
  }
  double e = 0;
  if (has) {
    load3(new_points + 3 * (size_t)j, p);
    e = row_error(Q, a, b, p);
  }
  block_partial<WG>(e, part_new);
}

int check_args(const vus_point_priors* Q) {
  VUS_REQUIRE(Q != nullptr, "point priors are null");
  VUS_REQUIRE(Q->n >= 0 && Q->n_points >= 0 && Q->n_rows >= 0 && Q->n_rows <= Q->n && Q->n_rows <= Q->n_points &&
                  (Q->n == 0) == (Q->n_rows == 0),
              "bad sizes: n=%d n_points=%d n_rows=%d", Q->n, Q->n_points, Q->n_rows);
  VUS_REQUIRE(Q->n == 0 || (Q->row_point && Q->row_ptr && Q->mean && Q->w), "point prior arrays are null");
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_point_prior_work_doubles(const vus_point_priors* Q) {
  if (!Q || Q->n_rows < 0) return 0;
  return 2ll * cdiv(Q->n_rows, WG) + 8;
}

extern "C" int vus_point_prior_check(const vus_point_priors* Q, void* stream) {
  if (int rc = check_args(Q)) return rc;
  if (Q->n == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  std::vector<int> rp, ptr;
  std::vector<double> mean, w;
  if (int rc = read_back(Q->row_point, Q->n_rows, rp, st)) return rc;
  if (int rc = read_back(Q->row_ptr, (size_t)Q->n_rows + 1, ptr, st)) return rc;
  if (int rc = read_back(Q->mean, 3 * (size_t)Q->n, mean, st)) return rc;
  if (int rc = read_back(Q->w, 3 * (size_t)Q->n, w, st)) return rc;
  if (int rc = check_csr_rows(rp, ptr, Q->n_rows, Q->n, Q->n_points, "row_point", "landmark")) return rc;
  for (size_t k = 0; k < 3 * (size_t)Q->n; ++k) {
    if (int rc = check_factor_weight((int)(k / 3), w[k])) return rc;
    VUS_REQUIRE(std::isfinite(mean[k]), "factor %d: mean %g is not finite", (int)(k / 3), mean[k]);
  }
  return VUS_OK;
}

extern "C" int vus_point_prior_linearize(const vus_point_priors* Q, const double* points, double* V, double* gl,
                                         double* err, double* work, void* stream) {
  if (int rc = check_args(Q)) return rc;
  VUS_REQUIRE(err != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (Q->n == 0) return zero_out(err, 1, st);
  VUS_REQUIRE(points && V && gl && work, "null buffer");
  const int nb = cdiv(Q->n_rows, WG);
  point_prior_linearize_kernel<<<nb, WG, 0, st>>>(*Q, points, V, gl, work);
  vus::reduce_partials(work, nb, err, st);
  VUS_CHECK_LAUNCH("point_prior_linearize");
  return VUS_OK;
}

extern "C" int vus_point_prior_eval_step(const vus_point_priors* Q, const double* points, const double* dl,
                                         const double* new_points, double* out, double* work, void* stream) {
  if (int rc = check_args(Q)) return rc;
  VUS_REQUIRE(out != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (Q->n == 0) return zero_out(out, 2, st);
  VUS_REQUIRE(points && dl && new_points && work, "null buffer");
  const int nb = cdiv(Q->n_rows, WG);
  point_prior_eval_kernel<<<nb, WG, 0, st>>>(*Q, points, dl, new_points, work, work + nb);
  vus::reduce_partials(work, nb, out, st);
  vus::reduce_partials(work + nb, nb, out + 1, st);
  VUS_CHECK_LAUNCH("point_prior_eval_step");
  return VUS_OK;
}

extern "C" int vus_point_prior_error(const vus_point_priors* Q, const double* points, double* err, double* work,
                                     void* stream) {
  if (int rc = check_args(Q)) return rc;
  VUS_REQUIRE(err != nullptr, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (Q->n == 0) return zero_out(err, 1, st);
  VUS_REQUIRE(points && work, "null buffer");
  const int nb = cdiv(Q->n_rows, WG);
  point_prior_eval_kernel<<<nb, WG, 0, st>>>(*Q, nullptr, nullptr, points, nullptr, work + nb);
  vus::reduce_partials(work + nb, nb, err, st);
  VUS_CHECK_LAUNCH("point_prior_error");
  return VUS_OK;
}
