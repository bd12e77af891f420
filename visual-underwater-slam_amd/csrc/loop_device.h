// loop_device.h -- device helpers shared by the two loop-closure units, loop.hip (vus_stereo_pair_pose, include/vus_loop.h)
// and pair_bundle.hip (vus_stereo_pair_bundle, include/vus_pair_bundle.h): the candidate rule, the fixed reduction tree of
// the per-pair sums and the 6 x 6 Cholesky solve.  Internal linkage: each unit gets its own copy, built with its own flags
// (-ffp-contract=off in both).
#pragma once
#include "vus_common.h"
#include <cmath>

namespace {

constexpr int LP_THREADS = 256;                  // one lane per hypothesis at the default n_hyp
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_SUMS = 28;                      // 21 of H (upper triangle, row-major), 6 of g, rss

struct LpCam {
  double fx, fy, cx, cy, fb, thr2;
};

// what a pair reads: its row of the match table, the stereo rows and key rows of its two frames, the clamped counts
struct LpPair {
  const int32_t* mt;        // may alias the output row
  const int32_t *sa, *sb;
  const int32_t *qa, *qb;   // Q8 only: the disp_q8 rows of the two frames
  const uint32_t *kla, *kra, *klb, *krb;
  int nla, nra, nlb, nrb;
};

struct LpCand {
  double Px, Py, Pz;
  float u, v;
  int d2, j;                // d2: pixels, or 1/256 px (Q8)
  uint32_t p1, p2;          // the positions y * W + x of the two left keypoints
  int d1;                   // as d2, in a
};

__device__ __forceinline__ void lp_point(double x, double y, double d, const LpCam& c, double& X, double& Y, double& Z) {
  Z = c.fb / d;
  X = ((x - c.cx) * Z) / c.fx;
  Y = ((y - c.cy) * Z) / c.fy;
}

// a disparity as the double lp_point divides by: d / 256.0 is exact, and 256 d0 / 256.0 is d0
template <bool Q8>
__device__ __forceinline__ double lp_disparity(int d) {
  if constexpr (Q8) return (double)d / 256.0;
  else return (double)d;
}

// slot i of the pair: false unless it is a candidate.  Every index is checked against its clamped count before it is used.
template <bool Q8>
__device__ __forceinline__ bool lp_candidate(const LpPair& p, int i, uint32_t W, const LpCam& c, LpCand& o) {
  if (i >= p.nla) return false;
  const int j = p.mt[i];
  if (j < 0 || j >= p.nlb) return false;
  const int ra = p.sa[i], rb = p.sb[j];
  if (ra < 0 || ra >= p.nra || rb < 0 || rb >= p.nrb) return false;
  const uint32_t p1 = p.kla[i] & VUS_KEY_POS_MASK, q1 = p.kra[ra] & VUS_KEY_POS_MASK;
  const uint32_t p2 = p.klb[j] & VUS_KEY_POS_MASK, q2 = p.krb[rb] & VUS_KEY_POS_MASK;
  const uint32_t y1 = p1 / W, x1 = p1 - y1 * W, xr1 = q1 - (q1 / W) * W;
  const uint32_t y2 = p2 / W, x2 = p2 - y2 * W, xr2 = q2 - (q2 / W) * W;
  int d1, d2;
  if constexpr (Q8) {
    d1 = p.qa[i];
    d2 = p.qb[j];
    if (d1 < 256 || d2 < 256) return false;
  } else {
    d1 = (int)x1 - (int)xr1;
    d2 = (int)x2 - (int)xr2;
    if (d1 < 1 || d2 < 1) return false;
  }
  lp_point((double)x1, (double)y1, lp_disparity<Q8>(d1), c, o.Px, o.Py, o.Pz);
  o.u = (float)x2;
  o.v = (float)y2;
  o.d2 = d2;
  o.j = j;
  o.p1 = p1;
  o.p2 = p2;
  o.d1 = d1;
  return true;
}

// The tables of pair c = (a, b).  A pair whose a or b lies outside [0, n_frames), or with a == b, gets frame 0 and empty
// lists: it indexes nothing with such a value and has no candidates.  (stereo_pair_pose_kernel keeps these statements in
// its own body: through this function its two instantiations load their arguments in another order and allocate other
// registers, and they are held to the instructions they had before this header existed -- profiles/pair_bundle.md.)
template <bool Q8>
__device__ __forceinline__ LpPair lp_pair(const int32_t* match_idx, int c, int a, int b, const int32_t* __restrict__ stereo_idx,
                                          const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count,
                                          const int32_t* __restrict__ disp_q8, int n_frames, int max_kp) {
  const bool pair_ok = a >= 0 && a < n_frames && b >= 0 && b < n_frames && a != b;
  const int fa = pair_ok ? a : 0, fb = pair_ok ? b : 0;
  LpPair p;
  p.mt = match_idx + (size_t)c * max_kp;
  p.sa = stereo_idx + (size_t)fa * max_kp;
  p.sb = stereo_idx + (size_t)fb * max_kp;
  p.qa = Q8 ? disp_q8 + (size_t)fa * max_kp : nullptr;
  p.qb = Q8 ? disp_q8 + (size_t)fb * max_kp : nullptr;
  p.kla = kp_keys + (size_t)(2 * fa) * max_kp;
  p.kra = p.kla + max_kp;
  p.klb = kp_keys + (size_t)(2 * fb) * max_kp;
  p.krb = p.klb + max_kp;
  p.nla = pair_ok ? min(kp_count[2 * fa], max_kp) : 0;      // a negative count: no keypoint
  p.nra = pair_ok ? min(kp_count[2 * fa + 1], max_kp) : 0;
  p.nlb = pair_ok ? min(kp_count[2 * fb], max_kp) : 0;
  p.nrb = pair_ok ? min(kp_count[2 * fb + 1], max_kp) : 0;
  return p;
}

// The fixed tree of a pair's LP_SUMS sums: every thread brings its own partial sums (its candidates t, t + LP_THREADS, ...
// added in ascending order) and count; a butterfly over each wave, then the waves' sums left in s_red [LP_WAVES][LP_SUMS]
// for lp_total to add in order.  Returns the total count to every thread.  Ends with a barrier.  Two runs give the same
// bits; no atomics on doubles.
__device__ __forceinline__ int lp_reduce(double (&acc)[LP_SUMS], int cnt, double* s_red, int* s_cnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < LP_SUMS; ++q) acc[q] += __shfl_xor(acc[q], o);
    cnt += __shfl_xor(cnt, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                    // the previous pass's sums have been read
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < LP_SUMS; ++q) s_red[wave * LP_SUMS + q] = acc[q];
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < LP_WAVES; ++w) total += s_cnt[w];
  return total;
}

__device__ __forceinline__ double lp_total(const double* s_red, int q) {
  return ((s_red[q] + s_red[LP_SUMS + q]) + s_red[2 * LP_SUMS + q]) + s_red[3 * LP_SUMS + q];
}

// x = H^-1 g by Cholesky, H given as its upper triangle row-major; false at a pivot that is not > 0
__device__ bool lp_solve6(const double (&h)[21], const double (&g)[6], double (&x)[6]) {
  double A[6][6], L[6][6];
  int q = 0;
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int r = p; r < 6; ++r) {
      A[p][r] = h[q];
      A[r][p] = h[q++];
    }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) return false;
    L[j][j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return true;
}

}  // namespace
