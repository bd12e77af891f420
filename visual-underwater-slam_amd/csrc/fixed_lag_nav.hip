// fixed_lag_nav.hip -- the fixed-lag prior of an inertial window for gfx950 (MI355X), fp64 (include/vus_fixed_lag_nav.h): the
// dense prior over pose, velocity and bias of consecutive keyframes in the per-keyframe-bias layout (family
// `nav_window_prior`), n = 15 m rows:
//   nwp_delta     thread / (window keyframe, node kind): its 6, 3 or 6 entries of u -- Local(x0_i, x_i), v_i - v0_i or
//                 b_i - b0_i (+ the node's step) -- one vector per grid.y
//   nwp_rows      workgroup (one wave) / (row, vector): y_r = sum_k H_rk u_k, lane t over k = t, t + 64, ... ascending, then
//                 the fixed LDS tree of factor_common.h (block_partial).  One sweep over H per vector: a form that read each
//                 row once for both vectors of eval_step was measured and was not faster (profiles/fixed_lag_nav.md)
//   nwp_energy    thread / row: u_r (g_r + y_r / 2), the constant c as one more row, to the workgroup's partial; writes the
//                 gradient g + y where asked -> vus::reduce_partials in index order
//   nwp_assemble  thread / target element of Sband and gs: a plain load, add and store (each element has one owner); the
//                 padding coordinates of the velocity nodes have no thread
//   nwp_compact   thread / element of the compacted H and g
// Launches only: no workgroup waits for another, no flags, no atomics; every sum has a fixed order.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "device_util.h"
#include "se3_device.h"
#include "factor_common.h"
#include "band_index.h"
#include "../../include/vus_fixed_lag_nav.h"

namespace {

constexpr int WG = 256;
constexpr int RW = 64;            // nwp_rows: one wave per row
constexpr int KF = 15;            // tangent coordinates of a keyframe: 6 pose, 3 velocity, 6 bias
constexpr int MAX_M = 4096 / 3;   // the band kernels serve at most 4096 nodes

// first tangent coordinate and width of node kind 0 (pose), 1 (velocity), 2 (bias) inside a keyframe's 15
__host__ __device__ __forceinline__ int kind_off(int kind) { return kind == 0 ? 0 : (kind == 1 ? 6 : 9); }
__host__ __device__ __forceinline__ int kind_dim(int kind) { return kind == 1 ? 3 : 6; }

// U[v, 15 i + off(kind) ..]: the state (xa, va, ba) for v = 0 (plus the step dp of node 3 (first + i) + kind when dp is given)
// and (xb, vb, bb) for v = 1
__global__ __launch_bounds__(WG) void nwp_delta_kernel(vus_nav_window_prior P, const double* __restrict__ xa,
                                                       const double* __restrict__ va, const double* __restrict__ ba,
                                                       const double* __restrict__ dp, const double* __restrict__ xb,
                                                       const double* __restrict__ vb, const double* __restrict__ bb,
                                                       double* __restrict__ U) {
  const int t = blockIdx.x * WG + threadIdx.x, v = blockIdx.y;
  if (t >= 3 * P.m) return;
  const int i = t / 3, kind = t - 3 * i;
  const size_t kf = (size_t)(P.first + i);
  double* u = U + (size_t)KF * P.m * v + KF * i + kind_off(kind);
  const double* step = (v == 0 && dp != nullptr) ? dp + 6 * (3 * kf + kind) : nullptr;
  if (kind == 0) {
    double T0[12], T[12], xi[6];
    load12(P.x0 + 12 * (size_t)i, T0);
    load12((v == 0 ? xa : xb) + 12 * kf, T);
    pose_local(T0, T, xi);
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = step ? xi[k] + step[k] : xi[k];
  } else if (kind == 1) {
    const double* vel = (v == 0 ? va : vb) + 3 * kf;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                        // the padding coordinates 3 .. 5 of the step are not read
      const double x = vel[k] - P.v0[3 * (size_t)i + k];
      u[k] = step ? x + step[k] : x;
    }
  } else {
    const double* bias = (v == 0 ? ba : bb) + 6 * kf;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double x = bias[k] - P.b0[6 * (size_t)i + k];
      u[k] = step ? x + step[k] : x;
    }
  }
}

// Y[v, r] = sum_k H[r, k] U[v, k]
__global__ __launch_bounds__(RW) void nwp_rows_kernel(const double* __restrict__ H, int n, const double* __restrict__ U,
                                                      double* __restrict__ Y) {
  const int r = blockIdx.x, v = blockIdx.y;
  const double* h = H + (size_t)n * r;
  const double* u = U + (size_t)n * v;
  double acc = 0;
  for (int k = threadIdx.x; k < n; k += RW) acc += h[k] * u[k];
  block_partial<RW>(acc, Y + (size_t)n * v);
}

// part[v, block] = the block's share of c + sum_r u_r (g_r + y_r / 2); grad (vector 0 only) = g + y
__global__ __launch_bounds__(WG) void nwp_energy_kernel(const double* __restrict__ g, double c, int n, const double* __restrict__ U,
                                                        const double* __restrict__ Y, double* __restrict__ grad,
                                                        double* __restrict__ part) {
  const int r = blockIdx.x * WG + threadIdx.x, v = blockIdx.y;
  double e = 0;
  if (r < n) {
    const double u = U[(size_t)n * v + r], y = Y[(size_t)n * v + r], gr = g[r];
    e = u * (gr + 0.5 * y);
    if (grad != nullptr && v == 0) grad[r] = gr + y;
  } else if (r == n) {
    e = c;
  }
  block_partial<WG>(e, part + (size_t)gridDim.x * v);
}

// thread t < 36 (3 m)^2: element e of the block (window node a, window node b); then 18 m threads for gs
__global__ __launch_bounds__(WG) void nwp_assemble_kernel(vus_nav_window_prior P, const double* __restrict__ grad, int band,
                                                          double* __restrict__ Sband, double* __restrict__ gs) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const int nn = 3 * P.m, n = KF * P.m;
  const long long nblk = 36ll * nn * nn;
  if (t < nblk) {
    const int q = (int)(t / 36), e = (int)(t - 36ll * q);
    const int a = q / nn, b = q - nn * a;
    if (b > a || a - b > band) return;                   // the upper blocks are not stored; the host refuses 3 m - 1 > band
    const int r = e / 6, c = e - 6 * r;
    const int ka = a / 3, kinda = a - 3 * ka, kb = b / 3, kindb = b - 3 * kb;
    if (r >= kind_dim(kinda) || c >= kind_dim(kindb)) return;        // velocity padding: not ours
    const size_t row = (size_t)(KF * ka + kind_off(kinda) + r), col = (size_t)(KF * kb + kind_off(kindb) + c);
    Sband[bandidx::blk(band, 3 * P.first + a, 3 * P.first + b) + e] += P.H[row * n + col];
  } else if (t < nblk + 6ll * nn) {
    const int k = (int)(t - nblk), a = k / 6, r = k - 6 * a;
    const int ka = a / 3, kinda = a - 3 * ka;
    if (r >= kind_dim(kinda)) return;
    gs[6 * (size_t)(3 * P.first + a) + r] += grad[KF * ka + kind_off(kinda) + r];
  }
}

// row / column q of the compacted system -> that of the 18-per-keyframe one
__device__ __forceinline__ int expand18(int q) {
  const int k = q / KF, o = q - KF * k;
  return 18 * k + (o < 9 ? o : o + 3);
}

__global__ __launch_bounds__(WG) void nwp_compact_kernel(const double* __restrict__ H18, const double* __restrict__ g18, int w,
                                                         double* __restrict__ H15, double* __restrict__ g15) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const int n = KF * w;
  const long long nh = (long long)n * n;
  if (t < nh) {
    const int a = (int)(t / n), b = (int)(t - (long long)n * a);
    H15[t] = H18[(size_t)expand18(a) * (18 * (size_t)w) + expand18(b)];
  } else if (t < nh + n) {
    g15[t - nh] = g18[expand18((int)(t - nh))];
  }
}

int nwp_args(const vus_nav_window_prior* P) {
  VUS_REQUIRE(P != nullptr, "nav window prior is null");
  VUS_REQUIRE(P->m >= 1 && P->m <= MAX_M, "nav window prior: m=%d outside [1, %d]", P->m, MAX_M);
  VUS_REQUIRE(P->n_poses >= 1, "nav window prior: n_poses=%d must be >= 1", P->n_poses);
  VUS_REQUIRE(P->first >= 0 && P->first <= P->n_poses - P->m,
              "nav window prior: first=%d + m=%d exceeds n_poses=%d (or first < 0)", P->first, P->m, P->n_poses);
  VUS_REQUIRE(P->x0 && P->v0 && P->b0 && P->H && P->g, "nav window prior arrays are null");
  return VUS_OK;
}

int nwp_band(const vus_nav_window_prior* P, int band) {
  VUS_REQUIRE(band >= 0 && 3 * P->m - 1 <= band, "nav window prior: 3 m - 1 = %d exceeds the band of %d nodes", 3 * P->m - 1, band);
  return VUS_OK;
}

inline int nwp_blocks(int n) { return cdiv(n + 1, WG); }

// out[v] = error at vector v, for nvec vectors: U, Y [2, n] and the partials in work
void nwp_energy(const vus_nav_window_prior* P, int nvec, const double* xa, const double* va, const double* ba, const double* dp,
                const double* xb, const double* vb, const double* bb, double* grad, double* out, double* work, hipStream_t st) {
  const int n = KF * P->m, nb = nwp_blocks(n);
  double* U = work;
  double* Y = work + 2 * (size_t)n;
  double* part = work + 4 * (size_t)n;
  nwp_delta_kernel<<<dim3(cdiv(3 * P->m, WG), nvec), WG, 0, st>>>(*P, xa, va, ba, dp, xb, vb, bb, U);
  nwp_rows_kernel<<<dim3(n, nvec), RW, 0, st>>>(P->H, n, U, Y);
  nwp_energy_kernel<<<dim3(nb, nvec), WG, 0, st>>>(P->g, P->c, n, U, Y, grad, part);
  for (int v = 0; v < nvec; ++v) vus::reduce_partials(part + (size_t)nb * v, nb, out + v, st);
}

}  // namespace

extern "C" long long vus_nav_window_prior_work_doubles(const vus_nav_window_prior* P) {
  if (!P || P->m < 1 || P->m > MAX_M) return 0;
  return 4ll * KF * P->m + 2ll * nwp_blocks(KF * P->m) + 8;
}

extern "C" int vus_nav_window_prior_check(const vus_nav_window_prior* P, int band, void* stream) {
  if (int rc = nwp_args(P)) return rc;
  if (int rc = nwp_band(P, band)) return rc;
  VUS_REQUIRE(std::isfinite(P->c), "nav window prior: the constant c=%g is not finite", P->c);
  hipStream_t st = vus::as_stream(stream);
  const size_t m = (size_t)P->m, n = KF * m;
  std::vector<double> H, g, x0, v0, b0;
  if (int rc = read_back(P->H, n * n, H, st)) return rc;
  if (int rc = read_back(P->g, n, g, st)) return rc;
  if (int rc = read_back(P->x0, 12 * m, x0, st)) return rc;
  if (int rc = read_back(P->v0, 3 * m, v0, st)) return rc;
  if (int rc = read_back(P->b0, 6 * m, b0, st)) return rc;
  for (size_t k = 0; k < x0.size(); ++k) VUS_REQUIRE(std::isfinite(x0[k]), "nav window prior: x0 of keyframe %d is not finite", (int)(k / 12));
  for (size_t k = 0; k < v0.size(); ++k) VUS_REQUIRE(std::isfinite(v0[k]), "nav window prior: v0 of keyframe %d is not finite", (int)(k / 3));
  for (size_t k = 0; k < b0.size(); ++k) VUS_REQUIRE(std::isfinite(b0[k]), "nav window prior: b0 of keyframe %d is not finite", (int)(k / 6));
  for (size_t k = 0; k < n; ++k) VUS_REQUIRE(std::isfinite(g[k]), "nav window prior: g[%d] is not finite", (int)k);
  double hmax = 0.0;
  for (size_t k = 0; k < n * n; ++k) {
    VUS_REQUIRE(std::isfinite(H[k]), "nav window prior: H[%d, %d] is not finite", (int)(k / n), (int)(k % n));
    hmax = std::fmax(hmax, std::fabs(H[k]));
  }
  for (size_t a = 0; a < n; ++a) {
    VUS_REQUIRE(H[a * n + a] >= 0.0, "nav window prior: H has a negative diagonal entry %g at row %d", H[a * n + a], (int)a);
    for (size_t b = 0; b < a; ++b)
      VUS_REQUIRE(std::fabs(H[a * n + b] - H[b * n + a]) <= 1e-12 * hmax,
                  "nav window prior: H is not symmetric at (%d, %d): %g against %g", (int)a, (int)b, H[a * n + b], H[b * n + a]);
  }
  return VUS_OK;
}

extern "C" int vus_nav_window_prior_linearize(const vus_nav_window_prior* P, const double* poses, const double* vels,
                                              const double* biases, double* grad, double* err, double* work, void* stream) {
  if (int rc = nwp_args(P)) return rc;
  VUS_REQUIRE(poses && vels && biases && grad && err && work, "null buffer");
  nwp_energy(P, 1, poses, vels, biases, nullptr, poses, vels, biases, grad, err, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("nav_window_prior_linearize");
  return VUS_OK;
}

extern "C" int vus_nav_window_prior_assemble(const vus_nav_window_prior* P, const double* grad, int band, double* Sband, double* gs,
                                             void* stream) {
  if (int rc = nwp_args(P)) return rc;
  if (int rc = nwp_band(P, band)) return rc;
  VUS_REQUIRE(grad && Sband && gs, "null buffer");
  const long long nn = 3ll * P->m, threads = 36 * nn * nn + 6 * nn;
  nwp_assemble_kernel<<<cdiv(threads, WG), WG, 0, vus::as_stream(stream)>>>(*P, grad, band, Sband, gs);
  VUS_CHECK_LAUNCH("nav_window_prior_assemble");
  return VUS_OK;
}

extern "C" int vus_nav_window_prior_eval_step(const vus_nav_window_prior* P, const double* poses, const double* vels,
                                              const double* biases, const double* dp, const double* new_poses,
                                              const double* new_vels, const double* new_biases, double* out, double* work,
                                              void* stream) {
  if (int rc = nwp_args(P)) return rc;
  VUS_REQUIRE(poses && vels && biases && dp && new_poses && new_vels && new_biases && out && work, "null buffer");
  nwp_energy(P, 2, poses, vels, biases, dp, new_poses, new_vels, new_biases, nullptr, out, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("nav_window_prior_eval_step");
  return VUS_OK;
}

extern "C" int vus_nav_window_prior_error(const vus_nav_window_prior* P, const double* poses, const double* vels,
                                          const double* biases, double* err, double* work, void* stream) {
  if (int rc = nwp_args(P)) return rc;
  VUS_REQUIRE(poses && vels && biases && err && work, "null buffer");
  nwp_energy(P, 1, poses, vels, biases, nullptr, poses, vels, biases, nullptr, err, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("nav_window_prior_error");
  return VUS_OK;
}

extern "C" int vus_nav_window_prior_compact(const double* H18, const double* g18, int w, double* H15, double* g15, void* stream) {
  VUS_REQUIRE(w >= 1 && w <= MAX_M, "nav window prior compact: w=%d outside [1, %d]", w, MAX_M);
  VUS_REQUIRE(H18 && g18 && H15 && g15, "nav window prior compact: null buffer");
  const long long n = (long long)KF * w;
  nwp_compact_kernel<<<cdiv(n * n + n, WG), WG, 0, vus::as_stream(stream)>>>(H18, g18, w, H15, g15);
  VUS_CHECK_LAUNCH("nav_window_prior_compact");
  return VUS_OK;
}
