// fixed_lag.hip -- fixed-lag smoothing for gfx950 (MI355X), fp64 (include/vus_fixed_lag.h): the dense prior over a window of
// consecutive poses (family `window_prior`) and the marginalisation of the head of the reduced camera system.
//
// window prior, n = 6 m rows:
//   wp_delta     thread / window pose: u = Local(x0_i, x_i) (+ the pose's step), one vector per grid.y
//   wp_matvec    workgroup (one wave) / row: y_r = sum_k H_rk u_k, lane t over k = t, t + 64, ... ascending, then the fixed
//                LDS tree of factor_common.h (block_partial)
//   wp_energy    thread / row: u_r (g_r + y_r / 2), the constant c as one more row, to the workgroup's partial; writes the
//                gradient g + y where asked -> vus::reduce_partials in index order
//   wp_assemble  thread / target element of Sband and gs: a plain load, add and store (each element has one owner)
// marginalisation, N = 6 n_nodes rows and the gradient as row N of a dense lower triangle T [LD, LD] in `work`:
//   mg_expand    thread / element of T
//   per 48-column panel of the dropped nodes:
//   mg_factor    ONE workgroup: the panel's diagonal block in LDS, right-looking Cholesky, the pivot test that sets status
//   mg_trsm      thread / row below the panel: forward substitution against the block (its row staged in LDS)
//   mg_update    wave / 16 x 16 tile of the trailing lower triangle: T_ij -= sum_k P_ik P_jk on v_mfma_f64_16x16x4_f64
//   mg_finish    thread / element of H (mirrored from the lower triangle), g and quad
// Launches only: no workgroup waits for another, no flags, no atomics; every sum has a fixed order.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "device_util.h"
#include "se3_device.h"
#include "factor_common.h"
#include "band_index.h"
#include "../../include/vus_fixed_lag.h"

namespace {

constexpr int WG = 256;
constexpr int RW = 64;        // wp_matvec: one wave per row
constexpr int PW = 48;        // columns of a panel (8 nodes)
constexpr int LDP = PW + 1;   // LDS row stride of a panel block
constexpr int TS = 64;        // mg_trsm: rows per workgroup
constexpr int MAX_NODES = 4096;

// ---- window prior ---------------------------------------------------------------------------------------------------
// U[v, 6 i ..] = Local(x0_i, x_i), x = xa for v = 0 (plus the step dp of pose first + i when dp is given) and xb for v = 1
__global__ __launch_bounds__(WG) void wp_delta_kernel(vus_window_prior P, const double* __restrict__ xa,
                                                      const double* __restrict__ dp, const double* __restrict__ xb,
                                                      double* __restrict__ U) {
  const int i = blockIdx.x * WG + threadIdx.x, v = blockIdx.y;
  if (i >= P.m) return;
  double T0[12], T[12], xi[6];
  load12(P.x0 + 12 * (size_t)i, T0);
  load12((v == 0 ? xa : xb) + 12 * (size_t)(P.first + i), T);
  pose_local(T0, T, xi);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    if (v == 0 && dp != nullptr) xi[k] += dp[6 * (size_t)(P.first + i) + k];
    U[6 * (size_t)P.m * v + 6 * i + k] = xi[k];
  }
}

// Y[v, r] = sum_k H[r, k] U[v, k]
__global__ __launch_bounds__(RW) void wp_matvec_kernel(const double* __restrict__ H, int n, const double* __restrict__ U,
                                                       double* __restrict__ Y) {
  const int r = blockIdx.x, v = blockIdx.y;
  const double* h = H + (size_t)n * r;
  const double* u = U + (size_t)n * v;
  double acc = 0;
  for (int k = threadIdx.x; k < n; k += RW) acc += h[k] * u[k];
  block_partial<RW>(acc, Y + (size_t)n * v);
}

// part[v, block] = the block's share of c + sum_r u_r (g_r + y_r / 2); grad (vector 0 only) = g + y
__global__ __launch_bounds__(WG) void wp_energy_kernel(const double* __restrict__ g, double c, int n, const double* __restrict__ U,
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

__global__ __launch_bounds__(WG) void wp_assemble_kernel(vus_window_prior P, const double* __restrict__ grad, int band,
                                                         double* __restrict__ Sband, double* __restrict__ gs) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long nblk = 36ll * P.m * P.m;
  const int n = 6 * P.m;
  if (t < nblk) {
    const int q = (int)(t / 36), e = (int)(t - 36ll * q);
    const int a = q / P.m, b = q - P.m * a;
    if (b > a || a - b > band) return;                   // the upper blocks are not stored; the host refuses m - 1 > band
    const int r = e / 6, c = e - 6 * r;
    Sband[bandidx::blk(band, P.first + a, P.first + b) + e] += P.H[(size_t)(6 * a + r) * n + 6 * b + c];
  } else if (t < nblk + n) {
    const int k = (int)(t - nblk);
    gs[6 * (size_t)P.first + k] += grad[k];
  }
}

int wp_args(const vus_window_prior* P) {
  VUS_REQUIRE(P != nullptr, "window prior is null");
  VUS_REQUIRE(P->m >= 1 && P->m <= MAX_NODES, "window prior: m=%d outside [1, %d]", P->m, MAX_NODES);
  VUS_REQUIRE(P->n_poses >= 1, "window prior: n_poses=%d must be >= 1", P->n_poses);
  VUS_REQUIRE(P->first >= 0 && P->first <= P->n_poses - P->m, "window prior: first=%d + m=%d exceeds n_poses=%d (or first < 0)",
              P->first, P->m, P->n_poses);
  VUS_REQUIRE(P->x0 && P->H && P->g, "window prior arrays are null");
  return VUS_OK;
}

inline int wp_blocks(int n) { return cdiv(n + 1, WG); }

// out[v] = error at vector v, for nvec vectors: U, Y [2, n] and the partials in work
void wp_energy(const vus_window_prior* P, int nvec, const double* xa, const double* dp, const double* xb, double* grad,
               double* out, double* work, hipStream_t st) {
  const int n = 6 * P->m, nb = wp_blocks(n);
  double* U = work;
  double* Y = work + 2 * (size_t)n;
  double* part = work + 4 * (size_t)n;
  wp_delta_kernel<<<dim3(cdiv(P->m, WG), nvec), WG, 0, st>>>(*P, xa, dp, xb, U);
  wp_matvec_kernel<<<dim3(n, nvec), RW, 0, st>>>(P->H, n, U, Y);
  wp_energy_kernel<<<dim3(nb, nvec), WG, 0, st>>>(P->g, P->c, n, U, Y, grad, part);
  for (int v = 0; v < nvec; ++v) vus::reduce_partials(part + (size_t)nb * v, nb, out + v, st);
}

// ---- marginalisation ------------------------------------------------------------------------------------------------
// T [LD, LD]: the lower triangle of S (rows < N), the gradient as row N, zero elsewhere
__global__ __launch_bounds__(WG) void mg_expand_kernel(const double* __restrict__ Sband, const double* __restrict__ gs, int N,
                                                       int band, int LD, double* __restrict__ T) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  if (t >= (long long)LD * LD) return;
  const int i = (int)(t / LD), j = (int)(t - (long long)LD * i);
  double v = 0.0;
  if (i < N && j <= i) {
    const int ni = i / 6, nj = j / 6;
    if (ni - nj <= band) v = Sband[bandidx::blk(band, ni, nj) + 6 * (i - 6 * ni) + (j - 6 * nj)];
  } else if (i == N && j < N) {
    v = gs[j];
  }
  T[t] = v;
}

// the pw x pw block at (c0, c0) -> its Cholesky factor, in place; a pivot that is not > 0 sets status (the first one only)
// and is replaced by 1 so that the rest stays finite
__global__ __launch_bounds__(64) void mg_factor_kernel(double* __restrict__ T, int LD, int c0, int pw, int* __restrict__ status) {
  __shared__ double s[PW * LDP];
  const int i = threadIdx.x;
  if (i < pw)
    for (int j = 0; j <= i; ++j) s[i * LDP + j] = T[(size_t)(c0 + i) * LD + c0 + j];
  __syncthreads();
  for (int j = 0; j < pw; ++j) {
    double d = s[j * LDP + j];
    if (!(d > 0.0)) {
      if (i == 0 && status[0] == 0) status[0] = 1 + c0 + j;
      d = 1.0;
    }
    const double rd = sqrt(d);
    __syncthreads();                                     // every thread has read the pivot
    if (i == j) s[j * LDP + j] = rd;
    if (i > j && i < pw) s[i * LDP + j] /= rd;
    __syncthreads();
    if (i > j && i < pw) {
      const double lij = s[i * LDP + j];
      for (int k = j + 1; k <= i; ++k) s[i * LDP + k] -= lij * s[k * LDP + j];
    }
    __syncthreads();
  }
  if (i < pw)
    for (int j = 0; j <= i; ++j) T[(size_t)(c0 + i) * LD + c0 + j] = s[i * LDP + j];
}

// rows c0 + pw .. n_rows - 1, columns c0 .. c0 + pw - 1:  X L^T = A, in place
__global__ __launch_bounds__(TS) void mg_trsm_kernel(double* __restrict__ T, int LD, int c0, int pw, int n_rows) {
  __shared__ double sl[PW * LDP];
  __shared__ double sx[TS * LDP];
  for (int e = threadIdx.x; e < pw * pw; e += TS) {
    const int a = e / pw, b = e - pw * a;
    sl[a * LDP + b] = b <= a ? T[(size_t)(c0 + a) * LD + c0 + b] : 0.0;
  }
  __syncthreads();
  const int r = c0 + pw + blockIdx.x * TS + threadIdx.x;
  if (r >= n_rows) return;
  double* x = sx + threadIdx.x * LDP;
  double* row = T + (size_t)r * LD + c0;
  for (int j = 0; j < pw; ++j) {
    double a = row[j];
    for (int k = 0; k < j; ++k) a -= x[k] * sl[j * LDP + k];
    x[j] = a / sl[j * LDP + j];
  }
  for (int j = 0; j < pw; ++j) row[j] = x[j];
}

// the trailing lower triangle, rows and columns >= t0 = c0 + pw:  T_ij -= sum_{k < pw} T[i, c0 + k] T[j, c0 + k].
// Tiles are aligned to 16 in absolute indices (LD is a multiple of 16, the rows past the matrix are zero): block x = tile
// row, wave = tile column; elements of a tile left of or above t0, or above the diagonal, are not stored.
__global__ __launch_bounds__(256) void mg_update_kernel(double* __restrict__ T, int LD, int c0, int pw, int tile0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int I = tile0 + blockIdx.x, J = tile0 + 4 * blockIdx.y + wave;
  if (J > I) return;
  const int arow = lane & 15, kq = lane >> 4, t0 = c0 + pw;
  const double* pa = T + (size_t)(16 * I + arow) * LD + c0;        // A[arow][k] = P[16 I + arow][k]
  const double* pb = T + (size_t)(16 * J + arow) * LD + c0;        // B[k][arow] = P[16 J + arow][k]
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k = kq; k < 4 * ((pw + 3) / 4); k += 4) {     // the same trip count in every lane; columns past pw are zero
    const bool in = k < pw;
    const double a = in ? pa[k] : 0.0, b = in ? pb[k] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  // C/D layout (f64): col = lane & 15, row = (lane >> 4) + 4 * reg
  const int j = 16 * J + arow;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 16 * I + kq + 4 * r;
    if (i >= t0 && j >= t0 && j <= i) T[(size_t)i * LD + j] -= acc[r];
  }
}

__global__ __launch_bounds__(WG) void mg_finish_kernel(const double* __restrict__ T, int LD, int N, int K, double* __restrict__ H,
                                                       double* __restrict__ g, double* __restrict__ quad) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const int nr = N - K;
  const long long nh = (long long)nr * nr;
  if (t < nh) {
    const int a = (int)(t / nr), b = (int)(t - (long long)nr * a);
    const int i = K + (a > b ? a : b), j = K + (a > b ? b : a);
    H[t] = T[(size_t)i * LD + j];
  } else if (t < nh + nr) {
    g[t - nh] = T[(size_t)N * LD + K + (int)(t - nh)];
  } else if (t == nh + nr) {
    quad[0] = -T[(size_t)N * LD + N];
  }
}

inline int mg_ld(int n_nodes) { return 16 * ((6 * n_nodes + 1 + 15) / 16); }

int mg_sizes(int n_nodes, int band, int n_drop) {
  VUS_REQUIRE(n_nodes >= 2 && n_nodes <= MAX_NODES, "band marginalize: n_nodes=%d outside [2, %d]", n_nodes, MAX_NODES);
  VUS_REQUIRE(band >= 0 && band < n_nodes, "band marginalize: band=%d outside [0, n_nodes=%d)", band, n_nodes);
  VUS_REQUIRE(n_drop >= 1 && n_drop < n_nodes, "band marginalize: n_drop=%d outside [1, n_nodes=%d)", n_drop, n_nodes);
  VUS_REQUIRE(n_nodes - n_drop <= band + 1, "band marginalize: the tail of %d nodes is wider than band + 1 = %d", n_nodes - n_drop,
              band + 1);
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_window_prior_work_doubles(const vus_window_prior* P) {
  if (!P || P->m < 1 || P->m > MAX_NODES) return 0;
  return 24ll * P->m + 2ll * wp_blocks(6 * P->m) + 8;
}

extern "C" int vus_window_prior_check(const vus_window_prior* P, int band, void* stream) {
  if (int rc = wp_args(P)) return rc;
  VUS_REQUIRE(band >= 0 && P->m - 1 <= band, "window prior: m - 1 = %d exceeds the band of %d nodes", P->m - 1, band);
  VUS_REQUIRE(std::isfinite(P->c), "window prior: the constant c=%g is not finite", P->c);
  hipStream_t st = vus::as_stream(stream);
  const size_t n = 6 * (size_t)P->m;
  std::vector<double> H, g, x0;
  if (int rc = read_back(P->H, n * n, H, st)) return rc;
  if (int rc = read_back(P->g, n, g, st)) return rc;
  if (int rc = read_back(P->x0, 12 * (size_t)P->m, x0, st)) return rc;
  for (size_t k = 0; k < x0.size(); ++k) VUS_REQUIRE(std::isfinite(x0[k]), "window prior: x0 of pose %d is not finite", (int)(k / 12));
  for (size_t k = 0; k < n; ++k) VUS_REQUIRE(std::isfinite(g[k]), "window prior: g[%d] is not finite", (int)k);
  double hmax = 0.0;
  for (size_t k = 0; k < n * n; ++k) {
    VUS_REQUIRE(std::isfinite(H[k]), "window prior: H[%d, %d] is not finite", (int)(k / n), (int)(k % n));
    hmax = std::fmax(hmax, std::fabs(H[k]));
  }
  for (size_t a = 0; a < n; ++a) {
    VUS_REQUIRE(H[a * n + a] >= 0.0, "window prior: H has a negative diagonal entry %g at row %d", H[a * n + a], (int)a);
    for (size_t b = 0; b < a; ++b)
      VUS_REQUIRE(std::fabs(H[a * n + b] - H[b * n + a]) <= 1e-12 * hmax, "window prior: H is not symmetric at (%d, %d): %g against %g",
                  (int)a, (int)b, H[a * n + b], H[b * n + a]);
  }
  return VUS_OK;
}

extern "C" int vus_window_prior_linearize(const vus_window_prior* P, const double* poses, double* grad, double* err, double* work,
                                          void* stream) {
  if (int rc = wp_args(P)) return rc;
  VUS_REQUIRE(poses && grad && err && work, "null buffer");
  wp_energy(P, 1, poses, nullptr, poses, grad, err, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("window_prior_linearize");
  return VUS_OK;
}

extern "C" int vus_window_prior_assemble(const vus_window_prior* P, const double* grad, int band, double* Sband, double* gs,
                                         void* stream) {
  if (int rc = wp_args(P)) return rc;
  VUS_REQUIRE(band >= 0 && P->m - 1 <= band, "window prior: m - 1 = %d exceeds the band of %d nodes", P->m - 1, band);
  VUS_REQUIRE(grad && Sband && gs, "null buffer");
  const long long threads = 36ll * P->m * P->m + 6ll * P->m;
  wp_assemble_kernel<<<cdiv(threads, WG), WG, 0, vus::as_stream(stream)>>>(*P, grad, band, Sband, gs);
  VUS_CHECK_LAUNCH("window_prior_assemble");
  return VUS_OK;
}

extern "C" int vus_window_prior_eval_step(const vus_window_prior* P, const double* poses, const double* dp, const double* new_poses,
                                          double* out, double* work, void* stream) {
  if (int rc = wp_args(P)) return rc;
  VUS_REQUIRE(poses && dp && new_poses && out && work, "null buffer");
  wp_energy(P, 2, poses, dp, new_poses, nullptr, out, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("window_prior_eval_step");
  return VUS_OK;
}

extern "C" int vus_window_prior_error(const vus_window_prior* P, const double* poses, double* err, double* work, void* stream) {
  if (int rc = wp_args(P)) return rc;
  VUS_REQUIRE(poses && err && work, "null buffer");
  wp_energy(P, 1, poses, nullptr, poses, nullptr, err, work, vus::as_stream(stream));
  VUS_CHECK_LAUNCH("window_prior_error");
  return VUS_OK;
}

extern "C" long long vus_ba_band_marginalize_work_doubles(int n_nodes, int band, int n_drop) {
  if (n_nodes < 2 || n_nodes > MAX_NODES || band < 0 || band >= n_nodes || n_drop < 1 || n_drop >= n_nodes ||
      n_nodes - n_drop > band + 1)
    return 0;
  const long long ld = mg_ld(n_nodes);
  return ld * ld;
}

extern "C" int vus_ba_band_marginalize(const double* Sband, int n_nodes, int band, const double* gs, int n_drop, double* H,
                                       double* g, double* quad, int* status, double* work, void* stream) {
  if (int rc = mg_sizes(n_nodes, band, n_drop)) return rc;
  VUS_REQUIRE(Sband && gs && H && g && quad && status && work, "band marginalize: null buffer");
  hipStream_t st = vus::as_stream(stream);
  const int N = 6 * n_nodes, K = 6 * n_drop, LD = mg_ld(n_nodes);
  VUS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
  mg_expand_kernel<<<cdiv((long long)LD * LD, WG), WG, 0, st>>>(Sband, gs, N, band, LD, work);
  for (int c0 = 0; c0 < K; c0 += PW) {
    const int pw = K - c0 < PW ? K - c0 : PW, t0 = c0 + pw;
    mg_factor_kernel<<<1, 64, 0, st>>>(work, LD, c0, pw, status);
    mg_trsm_kernel<<<cdiv(N + 1 - t0, TS), TS, 0, st>>>(work, LD, c0, pw, N + 1);
    const int tile0 = t0 / 16, nt = LD / 16 - tile0;
    mg_update_kernel<<<dim3(nt, cdiv(nt, 4)), 256, 0, st>>>(work, LD, c0, pw, tile0);
  }
  const long long nr = N - K;
  mg_finish_kernel<<<cdiv(nr * nr + nr + 1, WG), WG, 0, st>>>(work, LD, N, K, H, g, quad);
  VUS_CHECK_LAUNCH("band_marginalize");
  return VUS_OK;
}
