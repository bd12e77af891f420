// band_resolve.hip -- further right-hand sides against the factor band_solve.hip has left in Sband, on gfx950 (MI355X),
// fp64: X <- (L L^T)^-1 X for up to 384 columns (include/vus_closure.h: the Z = B^-1 U of a long loop closure).
//
//   resolve_kernel   block / 16 columns   forward sweep over all panels, then the backward sweep, alone: a workgroup
//                                         reads L (shared, read-only, L2) and its own 16 rows of X, nothing else
// A panel step of either sweep:
//   t  = x_P - A y          A = the 48 rows of the panel against the <= band nodes left of it (forward), or the
//                           transposed <= band + 7 node rows below it against the panel's 48 columns (backward); y = the
//                           part of X already solved.  v_mfma_f64_16x16x4_f64, K split over the four waves in chunks
//                           of KC rows of y staged in LDS, the waves' partial sums added in a fixed order
//   x_P = L_PP^-1 t  /  L_PP^-T t     the inverted panel as a 48 x 48 by 48 x 16 product (band >= 7 nodes), else a
//                           substitution with the factor (one thread per column)
// Every address inside L comes from band_index.h (rs_*), swept on the CPU by tests/native/band_resolve_check.cpp.
#include "vus_common.h"
#include "band_index.h"
#include "../../include/vus_closure.h"

namespace {

constexpr int PB = bandidx::PB;      // nodes per panel
constexpr int NB = bandidx::NB;      // scalar rows per panel
constexpr int NC = 16;               // columns per workgroup = the N of one MFMA tile
constexpr int KC = 192;              // rows of y staged per chunk (48 MFMA steps, 12 per wave)
constexpr int LDY = NC + 1;          // LDS row stride of a [rows][16] tile
constexpr int LDA = NB + 1;          // LDS row stride of the 48 x 48 diagonal block
constexpr int RS_THREADS = 256;
typedef double double4_t __attribute__((ext_vector_type(4)));
static_assert(KC % 16 == 0 && KC * LDY >= 4 * NB * NC, "the chunk buffer also holds the four waves' partial tiles");

template <bool BACKWARD>
__device__ __forceinline__ void panel_step(const double* __restrict__ L, int n, int band, int inverted, double* Xc,
                                           size_t ld, int cols, int p, double* sBuf, double* sT, double* sD) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int arow = lane & 15, kq = lane >> 4;
  const int k0 = PB * p;
  const int nb = 6 * min(PB, n - k0);
  // y rows the step multiplies with: X rows [y0, y0 + nK)
  const int y0 = BACKWARD ? 6 * (k0 + PB) : 6 * bandidx::rs_left_start(band, k0);
  const int nK = BACKWARD ? bandidx::rs_below_rows(band, n, k0) : 6 * k0 - y0;

  // the panel's diagonal block, dense (zero where nothing is stored)
  for (int e = tid; e < NB * NB; e += RS_THREADS) {
    const int r = e / NB, c = e - NB * r;
    const long long o = bandidx::rs_diag(band, k0, nb, r, c);
    sD[r * LDA + c] = o >= 0 ? L[o] : 0.0;
  }

  double4_t acc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) acc[a] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < nK; c0 += KC) {
    const int kc = min(KC, nK - c0);
    __syncthreads();
    for (int e = tid; e < KC * NC; e += RS_THREADS) {
      const int q = e / KC, K = e - KC * q;
      sBuf[K * LDY + q] = (K < kc && q < cols) ? Xc[q * ld + (size_t)(y0 + c0 + K)] : 0.0;
    }
    __syncthreads();
    const int n_steps = (kc + 3) / 4;
    for (int s = wave; s < n_steps; s += 4) {
      const int K = 4 * s + kq;
      const double b = sBuf[K * LDY + arow];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int R = 16 * a + arow;
        const long long o = BACKWARD ? bandidx::rs_below(band, n, k0, R, c0 + K) : bandidx::rs_left(band, n, k0, R, c0 + K);
        const double v = o >= 0 ? L[o] : 0.0;
        acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, b, acc[a], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  // C/D layout (f64): col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) sBuf[(wave * NB + 16 * a + kq + 4 * r) * NC + arow] = acc[a][r];
  __syncthreads();
  for (int e = tid; e < NB * NC; e += RS_THREADS) {
    const int q = e / NB, R = e - NB * q;
    const double sum = (sBuf[R * NC + q] + sBuf[(NB + R) * NC + q]) + (sBuf[(2 * NB + R) * NC + q] + sBuf[(3 * NB + R) * NC + q]);
    const double x = (R < nb && q < cols) ? Xc[q * ld + (size_t)(6 * k0 + R)] : 0.0;
    sT[R * LDY + q] = x - sum;
  }
  __syncthreads();
  // x_P into sBuf [48][LDY]
  if (inverted) {
    if (wave < 3) {
      double4_t z = double4_t{0.0, 0.0, 0.0, 0.0};
      const int R = 16 * wave + arow;
#pragma unroll
      for (int s = 0; s < NB / 4; ++s) {
        const int K = 4 * s + kq;
        const double v = BACKWARD ? sD[K * LDA + R] : sD[R * LDA + K];
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(v, sT[K * LDY + arow], z, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) sBuf[(16 * wave + kq + 4 * r) * LDY + arow] = z[r];
    }
  } else if (tid < NC) {
    // narrow bands: the factor itself.  Column tid, forward: rows 0 .. nb - 1 of L_PP; backward: rows nb - 1 .. 0 of L_PP^T
    for (int j = 0; j < nb; ++j) {
      const int r = BACKWARD ? nb - 1 - j : j;
      double v = sT[r * LDY + tid];
      if (BACKWARD) {
        for (int c = nb - 1; c > r; --c) v -= sD[c * LDA + r] * sBuf[c * LDY + tid];
      } else {
        for (int c = 0; c < r; ++c) v -= sD[r * LDA + c] * sBuf[c * LDY + tid];
      }
      sBuf[r * LDY + tid] = v / sD[r * LDA + r];
    }
  }
  __syncthreads();
  for (int e = tid; e < NB * NC; e += RS_THREADS) {
    const int q = e / NB, R = e - NB * q;
    if (R < nb && q < cols) Xc[q * ld + (size_t)(6 * k0 + R)] = sBuf[R * LDY + q];
  }
  __syncthreads();      // the rows just written are the next step's y; sBuf, sT and sD are free again
}

__global__ __launch_bounds__(RS_THREADS) void resolve_kernel(const double* __restrict__ L, int n, int band, int inverted,
                                                             double* X, int n_cols) {
  __shared__ double sBuf[KC * LDY];
  __shared__ double sT[NB * LDY];
  __shared__ double sD[NB * LDA];
  const size_t ld = 6 * (size_t)n;
  const int col0 = NC * blockIdx.x;
  const int cols = min(NC, n_cols - col0);
  double* Xc = X + (size_t)col0 * ld;
  const int NP = (n + PB - 1) / PB;
  for (int p = 0; p < NP; ++p) panel_step<false>(L, n, band, inverted, Xc, ld, cols, p, sBuf, sT, sD);
  for (int p = NP - 1; p >= 0; --p) panel_step<true>(L, n, band, inverted, Xc, ld, cols, p, sBuf, sT, sD);
}

}  // namespace

extern "C" int vus_ba_band_resolve(const double* L, int n_nodes, int band, double* X, int n_cols, double* work,
                                   long long work_doubles, void* stream) {
  VUS_REQUIRE(L && X, "null buffer");
  VUS_REQUIRE(n_nodes >= 1, "n_nodes=%d", n_nodes);
  VUS_REQUIRE(band >= 0 && band < n_nodes + 1, "band=%d against %d nodes", band, n_nodes);
  VUS_REQUIRE(n_cols >= 1 && n_cols <= VUS_CLOSURE_MAX_COLS, "n_cols=%d out of range [1, %d]", n_cols, VUS_CLOSURE_MAX_COLS);
  VUS_REQUIRE(work_doubles >= 0 && (work || work_doubles == 0), "work is null or work_doubles=%lld is negative", work_doubles);
  const double* Lend = L + bandidx::band_doubles(n_nodes, band);
  const double* Xend = X + (size_t)n_cols * 6 * n_nodes;
  VUS_REQUIRE(Xend <= L || Lend <= X, "X overlaps the factor");
  resolve_kernel<<<cdiv(n_cols, NC), RS_THREADS, 0, vus::as_stream(stream)>>>(L, n_nodes, band, band >= PB - 1 ? 1 : 0, X, n_cols);
  VUS_CHECK_LAUNCH("ba_band_resolve");
  return VUS_OK;
}
