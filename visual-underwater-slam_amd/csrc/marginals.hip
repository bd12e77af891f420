// marginals.hip -- marginal covariances of the bundle adjustment on gfx950 (MI355X), fp64: what
// gtsam.Marginals(graph, values).marginalCovariance(key) computes, from the reduced camera system S of ba.hip
// as band_solve.hip has factored it.
//
//   selinv_prep     block / panel      dense L_PP^-1 of every 8-node diagonal panel (read from the inverted panel the band
//                                      solve leaves for bands >= 7 nodes, inverted here by substitution for narrower ones)
//   selinv_x        block / 48 rows    X = L_RP L_PP^-1 of every panel (depends on L only: one launch for all panels)
//   selinv_gemm     block / (tile, K chunk)   partial sums of Sigma_RR X on v_mfma_f64_16x16x4_f64 (the hot path)
//   selinv_panel    block / 48 rows    Sigma_RP = -sum of the partials, stored where the band holds it; M_I = X_I^T Sigma_RP,I
//   selinv_pp       one block          Sigma_PP = L_PP^-T L_PP^-1 - sum_I M_I
//   point_cov_*     V^-1 + sum Y^T Sigma Y per landmark along the tile pairs of vus_ba_tiles; V positive-definiteness
//   border_*        the shared-bias border of graphs with inertial factors (rank-6 update of the band)
// Layouts and the recursion: include/vus_marginals.h, DESIGN.md "Marginal covariances".
#include "vus_common.h"
#include "band_index.h"
#include "factor_common.h"
#include "../../include/vus_marginals.h"

namespace {

constexpr int PB = bandidx::PB;      // nodes per panel
constexpr int NB = bandidx::NB;      // scalar columns per panel
constexpr int LDA = NB + 1;          // LDS row stride of a 48 x 48 tile
typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long blk(int band, int i, int k) { return bandidx::blk(band, i, k); }

// ---- dense L_PP^-1 of every panel: Linv [NP][48][48] row-major, zero outside the panel's nb x nb lower triangle ------
__global__ __launch_bounds__(64) void selinv_prep_kernel(const double* __restrict__ L, int n, int band, int inverted,
                                                        double* __restrict__ Linv) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int k0 = PB * p;
  const int nb = 6 * min(PB, n - k0);
  __shared__ double sL[NB * LDA];
  __shared__ double sI[NB * LDA];
  for (int t = lane; t < NB * LDA; t += 64) sL[t] = sI[t] = 0.0;
  __syncthreads();
  for (int t = lane; t < bandidx::DIAG_ELEMS; t += 64) {
    const long long o = bandidx::diag_elem(band, k0, nb, t);
    if (o < 0) continue;
    int r6, sd, e;
    bandidx::diag_slot(t, r6, sd, e);
    const int r = e / 6, c = e % 6;
    if (sd == 0 && c > r) continue;                   // the upper triangle of a diagonal block is not part of L
    sL[(6 * r6 + r) * LDA + 6 * (r6 - sd) + c] = L[o];
  }
  __syncthreads();
  if (inverted) {
    for (int t = lane; t < NB * LDA; t += 64) sI[t] = sL[t];
  } else if (lane < nb) {
    // column `lane` of the inverse by forward substitution (as diag_invert_kernel of band_solve.hip)
    double x[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      double acc = r == lane ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < r; ++k) acc -= sL[r * LDA + k] * x[k];
      x[r] = (r >= lane && r < nb) ? acc / sL[r * LDA + r] : 0.0;
      sI[r * LDA + lane] = x[r];
    }
  }
  __syncthreads();
  double* out = Linv + (size_t)p * NB * NB;
  for (int t = lane; t < NB * NB; t += 64) {
    const int r = t / NB, c = t % NB;
    out[t] = (r < nb && c < nb && c <= r) ? sI[r * LDA + c] : 0.0;
  }
}

// ---- X = L_RP L_PP^-1 for every panel: X [NP][6 BR][48], BR = rows of R rounded up to the panel; rows outside R zero ---
// block (p, t) = rows 8t .. 8t + 7 of R(p) = nodes k0 + 8 + 8t + ii.  L(i, k) of a block left of i's panel is stored
// TRANSPOSED: element (r, c) at blk(i, k) + 6 c + r.
__global__ __launch_bounds__(256) void selinv_x_kernel(const double* __restrict__ L, int n, int band, int br,
                                                      const double* __restrict__ Linv, double* __restrict__ X) {
  const int p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int k0 = PB * p, r0 = k0 + PB + PB * t;
  const int rend = min(n, k0 + PB + band);          // R = [k0 + 8, rend)
  __shared__ double sA[NB * LDA];
  __shared__ double sB[NB * LDA];
  double* out = X + ((size_t)p * br * 6 + (size_t)NB * t) * NB;
  if (r0 >= rend) {
    for (int e = tid; e < NB * NB; e += 256) out[e] = 0.0;
    return;
  }
  const double* li = Linv + (size_t)p * NB * NB;
  for (int e = tid; e < NB * NB; e += 256) {
    const int row = e / NB, col = e % NB;
    const int ii = row / 6, r = row % 6, kk = col / 6, c = col % 6;
    const int i = r0 + ii, k = k0 + kk;
    sA[row * LDA + col] = (i < rend && i - k <= band) ? L[blk(band, i, k) + 6 * c + r] : 0.0;
    sB[row * LDA + col] = li[e];
  }
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int row = e / NB, col = e % NB;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < NB; ++k) acc += sA[row * LDA + k] * sB[k * LDA + col];
    out[e] = acc;
  }
}

// ---- Sigma_RR X, partial over a chunk of K tiles, on the matrix cores --------------------------------------------------
// block (I, c): output rows 8I .. 8I + 7 of R, K tiles J = c, c + KC, ...  Sigma_RR(i, j) for i, j in R is always stored
// (|i - j| < band): block (i, j) at blk(i, j) row-major for i >= j, the transpose of blk(j, i) otherwise.
// The 48 x 48 output tile is nine 16 x 16 MFMA tiles; wave w owns tiles w, w + 4, w + 8.
__global__ __launch_bounds__(256) void selinv_gemm_kernel(const double* __restrict__ Sg, int n, int band, int k0,
                                                         const double* __restrict__ Xp, double* __restrict__ part,
                                                         int n_rt, int kc, int br) {
  const int I = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int R0 = k0 + PB, rend = min(n, k0 + PB + band);
  __shared__ double sA[NB * LDA];
  __shared__ double sB[NB * LDA];
  double4_t acc[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int arow = lane & 15, kq = lane >> 4;
  for (int J = c; J < n_rt; J += kc) {
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) {
      const int row = e / NB, col = e % NB;
      const int i = R0 + PB * I + row / 6, j = R0 + PB * J + col / 6;
      const int r = row % 6, cc = col % 6;
      double v = 0.0;
      if (i < rend && j < rend) v = i >= j ? Sg[blk(band, i, j) + 6 * r + cc] : Sg[blk(band, j, i) + 6 * cc + r];
      sA[row * LDA + col] = v;
      sB[row * LDA + col] = Xp[((size_t)NB * J + row) * NB + col];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int tt = wave + 4 * q;
      if (tt >= 9) break;
      const int a = tt / 3, b = tt % 3;
      const double* pa = sA + (16 * a + arow) * LDA + kq;      // A[16a + arow][4s + kq]
      const double* pb = sB + kq * LDA + 16 * b + arow;        // B[4s + kq][16b + arow]
#pragma unroll
      for (int s = 0; s < NB / 4; ++s)
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * s], pb[4 * s * LDA], acc[q], 0, 0, 0);
    }
  }
  // C/D layout (f64): col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = part + ((size_t)c * br * 6 + (size_t)NB * I) * NB;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int tt = wave + 4 * q;
    if (tt >= 9) break;
    const int a = tt / 3, b = tt % 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(size_t)(16 * a + kq + 4 * r) * NB + 16 * b + arow] = acc[q][r];
  }
}

// ---- Sigma_RP = -sum of the partials (stored where the band holds it), M_I = X_I^T Sigma_RP,I -> Mpart[I] ---------------
__global__ __launch_bounds__(256) void selinv_panel_kernel(double* __restrict__ Sg, int n, int band, int k0,
                                                          const double* __restrict__ Xp, const double* __restrict__ part,
                                                          int kc, int br, double* __restrict__ Mpart) {
  const int I = blockIdx.x, tid = threadIdx.x;
  const int R0 = k0 + PB, rend = min(n, k0 + PB + band);
  __shared__ double sS[NB * LDA];
  __shared__ double sX[NB * LDA];
  for (int e = tid; e < NB * NB; e += 256) {
    const int row = e / NB, col = e % NB;
    double s = 0.0;
    for (int c = 0; c < kc; ++c) s += part[((size_t)c * br * 6 + (size_t)NB * I + row) * NB + col];
    s = -s;
    sS[row * LDA + col] = s;
    sX[row * LDA + col] = Xp[((size_t)NB * I + row) * NB + col];
    const int i = R0 + PB * I + row / 6, k = k0 + col / 6;
    if (i < rend && i - k <= band) Sg[blk(band, i, k) + 6 * (row % 6) + col % 6] = s;
  }
  __syncthreads();
  double* out = Mpart + (size_t)I * NB * NB;
  for (int e = tid; e < NB * NB; e += 256) {
    const int a = e / NB, b = e % NB;
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < NB; ++r) acc += sX[r * LDA + a] * sS[r * LDA + b];
    out[e] = acc;
  }
}

// ---- Sigma_PP = L_PP^-T L_PP^-1 - sum_I M_I, symmetrised, every stored block of the panel written whole --------------
__global__ __launch_bounds__(256) void selinv_pp_kernel(double* __restrict__ Sg, int n, int band, int k0,
                                                       const double* __restrict__ Li, const double* __restrict__ Mpart,
                                                       int n_rt) {
  const int tid = threadIdx.x;
  __shared__ double sI[NB * LDA];
  __shared__ double sP[NB * LDA];
  for (int e = tid; e < NB * NB; e += 256) sI[(e / NB) * LDA + e % NB] = Li[e];
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int a = e / NB, b = e % NB;
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < NB; ++r) acc += sI[r * LDA + a] * sI[r * LDA + b];
    for (int t = 0; t < n_rt; ++t) acc -= Mpart[(size_t)t * NB * NB + e];
    sP[a * LDA + b] = acc;
  }
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int row = e / NB, col = e % NB;
    const int i = k0 + row / 6, k = k0 + col / 6;
    if (i < n && k <= i && i - k <= band)
      Sg[blk(band, i, k) + 6 * (row % 6) + col % 6] = 0.5 * (sP[row * LDA + col] + sP[col * LDA + row]);
  }
}

// ---- landmarks -----------------------------------------------------------------------------------------------------
// first_bad[0] = smallest landmark whose information V is not positive definite (leading minors of the 3 x 3, relative
// to its scale), untouched (0x7F7F7F7F from the caller's memset) if none
__global__ void point_check_kernel(int n_points, const double* __restrict__ V, int* __restrict__ first_bad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_points) return;
  const double* v = V + 6 * (size_t)j;
  const double a = v[0], b = v[1], c = v[2], d = v[3], e = v[4], f = v[5];
  const double scale = fmax(fabs(a), fmax(fabs(d), fabs(f)));
  const double m2 = a * d - b * b;
  const double m3 = a * (d * f - e * e) - b * (b * f - c * e) + c * (b * e - c * d);
  const double eps = 1e-13;
  const bool ok = scale > 0.0 && a > eps * scale && m2 > eps * scale * scale && m3 > eps * scale * scale * scale &&
                  isfinite(m3);
  if (!ok) atomicMin(first_bad, j);
}

__global__ void point_cov_init_kernel(int n_points, const double* __restrict__ Vinv, double* __restrict__ cov) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 9 * n_points) return;
  const int j = t / 9, e = t % 9;
  cov[t] = sym3(Vinv + 6 * (size_t)j, e / 3, e % 3);
}

// Y row of observation `o` (L-order): Y = W Vinv, 6 x 3
__device__ __forceinline__ void y_row(const double* __restrict__ W, const double* __restrict__ vi, int o, double* y) {
  const double* w = W + 18 * (size_t)o;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) y[3 * r + c] = w[3 * r] * sym3(vi, 0, c) + w[3 * r + 1] * sym3(vi, 1, c) + w[3 * r + 2] * sym3(vi, 2, c);
}

// One block per tile pair (I, I - d) of vus_ba_tiles: the 8 x 8 pose blocks of Sigma it covers are read ONCE into LDS,
// then one thread per landmark of the unit adds sum_{p in I, q in I - d} Y_p^T Sigma(p, q) Y_q (and its transpose for
// d > 0: the pairs (q, p)) to cov with f64 atomics.
__global__ __launch_bounds__(64) void point_cov_tiles_kernel(vus_ba_problem P, vus_ba_tiles T, const double* __restrict__ W,
                                                            const double* __restrict__ Vinv, const double* __restrict__ Sg,
                                                            int band_nodes, int ps, double* __restrict__ cov) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const int dt1 = (T.band + 7) / 8 + 1;
  const int I = u / dt1, d = u % dt1;
  const int e0 = T.unit_ptr[u], e1 = T.unit_ptr[u + 1];
  if (e0 == e1 || I - d < 0) return;
  __shared__ double sS[64 * 36];          // pose block (I*8 + a, (I-d)*8 + b) at 36 (8 a + b)
  const int pa0 = 8 * I, pb0 = 8 * (I - d);
  for (int t = tid; t < 64 * 36; t += 64) {
    const int ab = t / 36, e = t % 36, a = ab / 8, b = ab % 8;
    const int pi = pa0 + a, pk = pb0 + b;
    double v = 0.0;
    if (pi < P.n_poses && pk < P.n_poses) {
      const int ni = ps * pi, nk = ps * pk;
      if (ni >= nk && ni - nk <= band_nodes) v = Sg[blk(band_nodes, ni, nk) + e];
      else if (nk > ni && nk - ni <= band_nodes) v = Sg[blk(band_nodes, nk, ni) + 6 * (e % 6) + e / 6];
    }
    sS[t] = v;
  }
  __syncthreads();
  for (int en = e0 + tid; en < e1; en += 64) {
    const int4 ent = reinterpret_cast<const int4*>(T.entries)[en];
    const int ra = ent.x, rb = ent.y, j = ent.z;
    const unsigned ma = ent.w & 0xFF, mb = (ent.w >> 8) & 0xFF;
    const double* vi = Vinv + 6 * (size_t)j;
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int oa = ra;
    for (int a = 0; a < 8; ++a) {
      if (!((ma >> a) & 1)) continue;
      double ya[18];
      y_row(W, vi, oa++, ya);
      // Z = Y_a^T Sigma(a, b) for every b, then Z Y_b
      int ob = rb;
      for (int b = 0; b < 8; ++b) {
        if (!((mb >> b) & 1)) continue;
        double yb[18];
        y_row(W, vi, ob++, yb);
        const double* S = sS + 36 * (8 * a + b);
        double Z[18];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
          for (int cc = 0; cc < 6; ++cc) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) s += ya[3 * r + x] * S[6 * r + cc];
            Z[6 * x + cc] = s;
          }
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
          for (int y = 0; y < 3; ++y) {
            double s = 0.0;
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) s += Z[6 * x + cc] * yb[3 * cc + y];
            C[3 * x + y] += s;
          }
      }
    }
    double* o = cov + 9 * (size_t)j;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) atomicAdd(o + 3 * x + y, d > 0 ? C[3 * x + y] + C[3 * y + x] : C[3 * x + y]);
  }
}

// ---- bias border ---------------------------------------------------------------------------------------------------
// U = rhs[1..6] (A^-1 Scb), Sc = Sbb - Scb^T U, Sigma_bb = Sc^-1, T_i = U_i Sc^-1 (= -Sigma_nb(i)) in Snb
__global__ __launch_bounds__(1024) void border_sc_kernel(int n_nodes, const double* __restrict__ rhs,
                                                        const double* __restrict__ Scb, const double* __restrict__ Sbb,
                                                        double* __restrict__ Sigma_bb, double* __restrict__ ok) {
  const int tid = threadIdx.x;
  const size_t ld = 6 * (size_t)n_nodes;
  __shared__ double part[36][33];
  const int e = tid % 36, slot = tid / 36;        // 28 slots of 36 threads
  const int a = e / 6, b = e % 6;
  double s = 0.0;
  if (slot < 28)
    for (size_t row = slot; row < ld; row += 28) s += Scb[(row / 6) * 36 + 6 * (row % 6) + a] * rhs[(1 + b) * ld + row];
  if (slot < 28) part[e][slot] = s;
  __syncthreads();
  __shared__ double M[6][13];
  if (tid < 36) {
    double t = 0.0;
    for (int k = 0; k < 28; ++k) t += part[tid][k];
    M[tid / 6][tid % 6] = Sbb[tid] - t;
    M[tid / 6][6 + tid % 6] = (tid / 6 == tid % 6) ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    // positive-definiteness first: Cholesky of the symmetric part, every pivot > 1e-13 of the largest diagonal entry
    // (the criterion of point_check_kernel); then the inverse by Gauss-Jordan with partial pivoting on [Sc | I]
    bool good = true;
    double C[6][6], scale = 0.0;
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) C[r][c] = 0.5 * (M[r][c] + M[c][r]);
      scale = fmax(scale, fabs(C[r][r]));
    }
    for (int c = 0; c < 6 && good; ++c) {
      double d = C[c][c];
      for (int k = 0; k < c; ++k) d -= C[c][k] * C[c][k];
      if (!(d > 1e-13 * scale) || !isfinite(d)) { good = false; break; }
      const double l = sqrt(d);
      C[c][c] = l;
      for (int r = c + 1; r < 6; ++r) {
        double s = C[r][c];
        for (int k = 0; k < c; ++k) s -= C[r][k] * C[c][k];
        C[r][c] = s / l;
      }
    }
    for (int c = 0; c < 6 && good; ++c) {
      int pr = c;
      for (int r = c + 1; r < 6; ++r) if (fabs(M[r][c]) > fabs(M[pr][c])) pr = r;
      if (!(M[pr][c] > 0.0 || M[pr][c] < 0.0)) { good = false; break; }
      for (int k = 0; k < 12; ++k) { const double t = M[c][k]; M[c][k] = M[pr][k]; M[pr][k] = t; }
      const double inv = 1.0 / M[c][c];
      for (int k = 0; k < 12; ++k) M[c][k] *= inv;
      for (int r = 0; r < 6; ++r) {
        if (r == c) continue;
        const double f = M[r][c];
        for (int k = 0; k < 12; ++k) M[r][k] -= f * M[c][k];
      }
    }
    ok[0] = good ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid < 36) Sigma_bb[tid] = 0.5 * (M[tid / 6][6 + tid % 6] + M[tid % 6][6 + tid / 6]);
}

__global__ void border_nb_kernel(int n_nodes, const double* __restrict__ rhs, const double* __restrict__ Sigma_bb,
                                 double* __restrict__ Sigma_nb) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;      // (node i, row r, bias column q)
  if (t >= 36 * n_nodes) return;
  const int i = t / 36, r = (t % 36) / 6, q = t % 6;
  const size_t ld = 6 * (size_t)n_nodes;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) s += rhs[(1 + k) * ld + 6 * (size_t)i + r] * Sigma_bb[6 * k + q];
  Sigma_nb[t] = -s;
}

// Sigma(i, k) += U_i Sc^-1 U_k^T = -Sigma_nb(i) U_k^T for every stored block
__global__ void border_band_kernel(int n_nodes, int band, const double* __restrict__ rhs,
                                   const double* __restrict__ Sigma_nb, double* __restrict__ Sg) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36ll * n_nodes * (band + 1)) return;
  const long long bi = t / 36;
  const int e = (int)(t % 36), i = (int)(bi / (band + 1)), s = (int)(bi % (band + 1)), k = i - s;
  if (k < 0) return;
  const int r = e / 6, c = e % 6;
  const size_t ld = 6 * (size_t)n_nodes;
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) acc -= Sigma_nb[36 * (size_t)i + 6 * r + q] * rhs[(1 + q) * ld + 6 * (size_t)k + c];
  Sg[t] += acc;
}

struct SelinvPlan {
  int np, br, kc_max;
  size_t off_linv, off_x, off_part, off_m, total;
};
SelinvPlan selinv_plan(int n, int band) {
  SelinvPlan p;
  p.np = (n + PB - 1) / PB;
  const int brt = band > 0 ? (band + PB - 1) / PB : 1;     // row tiles of R
  p.br = PB * brt;
  p.kc_max = brt;
  p.off_linv = 0;
  p.off_x = p.off_linv + (size_t)p.np * NB * NB;
  p.off_part = p.off_x + (size_t)p.np * 6 * p.br * NB;
  p.off_m = p.off_part + (size_t)p.kc_max * 6 * p.br * NB;
  p.total = p.off_m + (size_t)brt * NB * NB;
  return p;
}

}  // namespace

extern "C" long long vus_ba_band_selinv_work_doubles(int n_nodes, int band) {
  if (n_nodes <= 0 || band < 0) return 0;
  return (long long)selinv_plan(n_nodes, band).total;
}

extern "C" int vus_ba_band_selinv(const double* L, int n_nodes, int band, double* Sigma, double* work,
                                  long long work_doubles, void* stream) {
  VUS_REQUIRE(L && Sigma && work, "null buffer");
  VUS_REQUIRE(n_nodes >= 1, "n_nodes=%d", n_nodes);
  VUS_REQUIRE(band >= 0 && band < n_nodes + 1, "band=%d against %d nodes", band, n_nodes);
  VUS_REQUIRE((const double*)Sigma != L, "Sigma must not alias the factor");
  const SelinvPlan pl = selinv_plan(n_nodes, band);
  VUS_REQUIRE(work_doubles >= (long long)pl.total, "work holds %lld doubles, %lld needed", work_doubles, (long long)pl.total);
  hipStream_t st = vus::as_stream(stream);
  VUS_CHECK_HIP(hipMemsetAsync(Sigma, 0, sizeof(double) * (size_t)bandidx::band_doubles(n_nodes, band), st));
  double* Linv = work + pl.off_linv;
  double* X = work + pl.off_x;
  double* part = work + pl.off_part;
  double* Mp = work + pl.off_m;
  selinv_prep_kernel<<<pl.np, 64, 0, st>>>(L, n_nodes, band, band >= PB - 1 ? 1 : 0, Linv);
  VUS_CHECK_LAUNCH("ba_band_selinv prep");
  selinv_x_kernel<<<dim3(pl.np, pl.br / PB), 256, 0, st>>>(L, n_nodes, band, pl.br, Linv, X);
  VUS_CHECK_LAUNCH("ba_band_selinv x");
  for (int p = pl.np - 1; p >= 0; --p) {
    const int k0 = PB * p;
    const int rend = n_nodes < k0 + PB + band ? n_nodes : k0 + PB + band;
    const int n_r = rend > k0 + PB ? rend - k0 - PB : 0;
    const int n_rt = (n_r + PB - 1) / PB;
    const double* Xp = X + (size_t)p * 6 * pl.br * NB;
    if (n_rt > 0) {
      // split K so that about 256 blocks share the product
      int kc = cdiv(256, n_rt);
      if (kc > n_rt) kc = n_rt;
      selinv_gemm_kernel<<<dim3(n_rt, kc), 256, 0, st>>>(Sigma, n_nodes, band, k0, Xp, part, n_rt, kc, pl.br);
      VUS_CHECK_LAUNCH("ba_band_selinv gemm");
      selinv_panel_kernel<<<n_rt, 256, 0, st>>>(Sigma, n_nodes, band, k0, Xp, part, kc, pl.br, Mp);
      VUS_CHECK_LAUNCH("ba_band_selinv panel");
    }
    selinv_pp_kernel<<<1, 256, 0, st>>>(Sigma, n_nodes, band, k0, Linv + (size_t)p * NB * NB, Mp, n_rt);
    VUS_CHECK_LAUNCH("ba_band_selinv diag");
  }
  return VUS_OK;
}

extern "C" int vus_ba_point_check(const double* V, int n_points, int* first_bad, void* stream) {
  VUS_REQUIRE(first_bad != nullptr, "first_bad is null");
  VUS_REQUIRE(n_points >= 0, "n_points=%d", n_points);
  VUS_REQUIRE(V || !n_points, "V is null");
  hipStream_t st = vus::as_stream(stream);
  VUS_CHECK_HIP(hipMemsetAsync(first_bad, 0x7F, sizeof(int), st));
  if (n_points == 0) return VUS_OK;
  point_check_kernel<<<cdiv(n_points, 256), 256, 0, st>>>(n_points, V, first_bad);
  VUS_CHECK_LAUNCH("ba_point_check");
  return VUS_OK;
}

extern "C" int vus_ba_point_covariance(const vus_ba_problem* P, const vus_ba_tiles* T, const double* W, const double* Vinv,
                                       const double* Sigma, int band_nodes, double* cov, void* stream) {
  VUS_REQUIRE(P != nullptr && T != nullptr, "problem or tile structure is null");
  const int nP = P->n_poses, nL = P->n_points, nO = P->n_obs;
  const int ps = P->pose_stride > 1 ? P->pose_stride : 1;
  VUS_REQUIRE(nP >= 1 && nL >= 0 && nO >= 0, "bad sizes: poses=%d points=%d obs=%d", nP, nL, nO);
  VUS_REQUIRE(Sigma != nullptr, "Sigma is null");
  VUS_REQUIRE((Vinv && cov) || !nL, "null landmark buffer");
  VUS_REQUIRE((W && P->point_ptr) || !nO, "null observation buffer");
  VUS_REQUIRE(T->band >= 0 && T->n_tiles == (nP + 7) / 8 && T->n_units == T->n_tiles * ((T->band + 7) / 8 + 1) &&
                  T->n_entries >= 0 && (T->unit_ptr || !T->n_units) && (T->entries || !T->n_entries),
              "tile structure of another problem: band=%d tiles=%d units=%d", T->band, T->n_tiles, T->n_units);
  VUS_REQUIRE(band_nodes >= ps * T->band && band_nodes < ps * nP + 1, "band_nodes=%d against %d poses of tile band, %d nodes",
              band_nodes, T->band, ps * nP);
  if (nL == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  point_cov_init_kernel<<<cdiv(9ll * nL, 256), 256, 0, st>>>(nL, Vinv, cov);
  VUS_CHECK_LAUNCH("ba_point_covariance init");
  if (T->n_entries > 0 && nO > 0) {
    point_cov_tiles_kernel<<<T->n_units, 64, 0, st>>>(*P, *T, W, Vinv, Sigma, band_nodes, ps, cov);
    VUS_CHECK_LAUNCH("ba_point_covariance tiles");
  }
  return VUS_OK;
}

extern "C" int vus_nav_border_covariance(int n_nodes, int band, const double* rhs, const double* Scb, const double* Sbb,
                                         double* Sigma, double* Sigma_nb, double* Sigma_bb, double* ok, void* stream) {
  VUS_REQUIRE(rhs && Scb && Sbb && Sigma && Sigma_nb && Sigma_bb && ok, "null buffer");
  VUS_REQUIRE(n_nodes >= 1, "n_nodes=%d", n_nodes);
  VUS_REQUIRE(band >= 0 && band < n_nodes + 1, "band=%d against %d nodes", band, n_nodes);
  hipStream_t st = vus::as_stream(stream);
  border_sc_kernel<<<1, 1024, 0, st>>>(n_nodes, rhs, Scb, Sbb, Sigma_bb, ok);
  VUS_CHECK_LAUNCH("nav_border_covariance sc");
  border_nb_kernel<<<cdiv(36ll * n_nodes, 256), 256, 0, st>>>(n_nodes, rhs, Sigma_bb, Sigma_nb);
  VUS_CHECK_LAUNCH("nav_border_covariance nb");
  border_band_kernel<<<cdiv(36ll * n_nodes * (band + 1), 256), 256, 0, st>>>(n_nodes, band, rhs, Sigma_nb, Sigma);
  VUS_CHECK_LAUNCH("nav_border_covariance band");
  return VUS_OK;
}
