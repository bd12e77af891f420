// pair_bundle.hip -- vus_stereo_pair_bundle (include/vus_pair_bundle.h): the second stage of a loop-closure measurement, a
// two-view refit behind vus_stereo_pair_pose(_q8).  The final inliers of stage one become free 3-D points, both stereo
// observations (x, y, d) of every point enter, and the pose comes from the Schur-reduced 6 x 6 system.
//
// One workgroup of 256 threads per pair, all fp64.  Thread t owns candidates t, t + 256, ...: a round is one pass over a
// thread's own points (their blocks formed and eliminated in registers), the fixed reduction tree of loop_device.h over
// 21 + 6 + 1 sums, the 6 x 6 solve on thread 0, and a second pass over the same points that recomputes their blocks for
// the back-substitution.  A point's position lives in the `points` output between the passes: only its owner touches it.
//
// Built with FRONTEND_FLAGS (-ffp-contract=off): every fp64 statement below is the header's, operation by operation, as
// the numpy restatement of the test suite (tests/pair_bundle_ref.py) writes it.  Do not fuse, reorder or "simplify" them.
#include "vus_common.h"
#include <cmath>
#include "se3_device.h"
#include "loop_device.h"
#include "../../include/vus_pair_bundle.h"

namespace {

constexpr int PB_LDS_PER_SLOT = 5 * (int)sizeof(uint32_t);      // two key positions, two disparity integers, the slot
constexpr uint32_t PB_ACTIVE = 0x80000000u;                     // on a slot word: the point was active in the last pass

struct PbWeights {
  double wu, wd, gate2;      // 1 / sigma_uv^2, 1 / sigma_d^2, gate^2
};

// what a compacted candidate keeps in LDS: enough to rebuild its two observations
struct PbLds {
  uint32_t *k1, *k2;         // y * W + x of the left keypoints in a and b
  int *d1, *d2;              // disparities: pixels, or 1/256 px (Q8)
  uint32_t* slot;            // its slot i of the match row, PB_ACTIVE or'ed in
};

template <bool Q8>
__device__ __forceinline__ void pb_observations(const PbLds& s, int m, uint32_t W, double (&za)[3], double (&zb)[3]) {
  const uint32_t p1 = s.k1[m], p2 = s.k2[m];
  const uint32_t y1 = p1 / W, x1 = p1 - y1 * W, y2 = p2 / W, x2 = p2 - y2 * W;
  za[0] = (double)x1; za[1] = (double)y1; za[2] = lp_disparity<Q8>(s.d1[m]);
  zb[0] = (double)x2; zb[1] = (double)y2; zb[2] = lp_disparity<Q8>(s.d2[m]);
}

// pi(Y) - z and the non-zero entries of D(Y) = d pi / dY: rows (a, 0, g), (0, b, h), (0, 0, k)
struct PbProj {
  double r[3];
  double a, b, g, h, k;
};

__device__ __forceinline__ PbProj pb_project(const double (&Y)[3], const double (&z)[3], const LpCam& c) {
  PbProj o;
  const double iz = 1.0 / Y[2], e = c.fb * iz, px = Y[0] * iz, py = Y[1] * iz;
  o.a = c.fx * iz;
  o.b = c.fy * iz;
  o.r[0] = (c.fx * px + c.cx) - z[0];
  o.r[1] = (c.fy * py + c.cy) - z[1];
  o.r[2] = e - z[2];
  o.g = -(o.a * px);
  o.h = -(o.b * py);
  o.k = -(e * iz);
  return o;
}

// sum over the three residual rows k of (w_k L[k]) R[k], added as ((k = 0) + (k = 1)) + (k = 2)
__device__ __forceinline__ double pb_dot3(const double (&wl)[3], double r0, double r1, double r2) {
  return (wl[0] * r0 + wl[1] * r1) + wl[2] * r2;
}

// The blocks of one point under the model T: its error e2, whether it lies in front of both cameras, A (upper triangle
// 00 01 02 11 12 22), B [3][6], C (upper triangle, row-major), gp, gt.  A caller that does not read C or gt does not pay
// for them (everything is inlined).
__device__ __forceinline__ void pb_blocks(const double (&T)[12], const double (&p)[3], const double (&za)[3],
                                          const double (&zb)[3], const LpCam& c, const PbWeights& w, double& e2, bool& front,
                                          double (&A)[6], double (&B)[3][6], double (&C)[21], double (&gp)[3],
                                          double (&gt)[6]) {
  double X[3];
  const double Dx = p[0] - T[9], Dy = p[1] - T[10], Dz = p[2] - T[11];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) X[cc] = (T[cc] * Dx + T[3 + cc] * Dy) + T[6 + cc] * Dz;
  const PbProj qa = pb_project(p, za, c), qb = pb_project(X, zb, c);
  front = p[2] > 0.0 && X[2] > 0.0;
  const double wk[3] = {w.wu, w.wu, w.wd};
  e2 = ((wk[0] * qa.r[0] * qa.r[0] + wk[1] * qa.r[1] * qa.r[1]) + wk[2] * qa.r[2] * qa.r[2]) +
       ((wk[0] * qb.r[0] * qb.r[0] + wk[1] * qb.r[1] * qb.r[1]) + wk[2] * qb.r[2] * qb.r[2]);
  // the Jacobians by residual row k: Ja = D(p), Jp = D(X) R^T, Jt = D(X) [ [X]x | -I ]
  const double Ja[3][3] = {{qa.a, 0.0, qa.g}, {0.0, qa.b, qa.h}, {0.0, 0.0, qa.k}};
  double Jp[3][3];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    Jp[0][cc] = qb.a * T[3 * cc] + qb.g * T[3 * cc + 2];
    Jp[1][cc] = qb.b * T[3 * cc + 1] + qb.h * T[3 * cc + 2];
    Jp[2][cc] = qb.k * T[3 * cc + 2];
  }
  const double Jt[3][6] = {{-(qb.g * X[1]), qb.g * X[0] - qb.a * X[2], qb.a * X[1], -qb.a, 0.0, -qb.g},
                           {qb.b * X[2] - qb.h * X[1], qb.h * X[0], -(qb.b * X[0]), 0.0, -qb.b, -qb.h},
                           {-(qb.k * X[1]), qb.k * X[0], 0.0, 0.0, 0.0, -qb.k}};
  int q = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double wa[3] = {wk[0] * Ja[0][r], wk[1] * Ja[1][r], wk[2] * Ja[2][r]};
    const double wp[3] = {wk[0] * Jp[0][r], wk[1] * Jp[1][r], wk[2] * Jp[2][r]};
#pragma unroll
    for (int cc = r; cc < 3; ++cc)
      A[q++] = pb_dot3(wa, Ja[0][cc], Ja[1][cc], Ja[2][cc]) + pb_dot3(wp, Jp[0][cc], Jp[1][cc], Jp[2][cc]);
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) B[r][cc] = pb_dot3(wp, Jt[0][cc], Jt[1][cc], Jt[2][cc]);
    gp[r] = pb_dot3(wa, qa.r[0], qa.r[1], qa.r[2]) + pb_dot3(wp, qb.r[0], qb.r[1], qb.r[2]);
  }
  q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double wt[3] = {wk[0] * Jt[0][r], wk[1] * Jt[1][r], wk[2] * Jt[2][r]};
#pragma unroll
    for (int cc = r; cc < 6; ++cc) C[q++] = pb_dot3(wt, Jt[0][cc], Jt[1][cc], Jt[2][cc]);
    gt[r] = pb_dot3(wt, qb.r[0], qb.r[1], qb.r[2]);
  }
}

// A = L L^T, A as its upper triangle 00 01 02 11 12 22, L as 00 10 11 20 21 22; false at a pivot that is not > 0
__device__ __forceinline__ bool pb_chol3(const double (&A)[6], double (&L)[6]) {
  if (!(A[0] > 0.0)) return false;
  L[0] = sqrt(A[0]);
  L[1] = A[1] / L[0];
  L[3] = A[2] / L[0];
  const double d1 = A[3] - L[1] * L[1];
  if (!(d1 > 0.0)) return false;
  L[2] = sqrt(d1);
  L[4] = (A[4] - L[3] * L[1]) / L[2];
  const double d2 = (A[5] - L[3] * L[3]) - L[4] * L[4];
  if (!(d2 > 0.0)) return false;
  L[5] = sqrt(d2);
  return true;
}

// x = A^-1 r from the factor of pb_chol3
__device__ __forceinline__ void pb_solve3(const double (&L)[6], double r0, double r1, double r2, double& x0, double& x1,
                                          double& x2) {
  const double y0 = r0 / L[0];
  const double y1 = (r1 - L[1] * y0) / L[2];
  const double y2 = ((r2 - L[3] * y0) - L[4] * y1) / L[5];
  x2 = y2 / L[5];
  x1 = (y1 - L[4] * x2) / L[2];
  x0 = ((y0 - L[1] * x1) - L[3] * x2) / L[0];
}

// One pass over the thread's own points: decides which are active (the slot word keeps the answer), eliminates them and
// sums S (upper triangle), g and e2; the waves' sums are left in s_red.  Returns the number of active points to every thread.
template <bool Q8>
__device__ __forceinline__ int pb_accumulate(const PbLds& s, int n, uint32_t W, const LpCam& c, const PbWeights& w,
                                             const double (&T)[12], const double* pts, double* s_red, int* s_cnt) {
  double acc[LP_SUMS];
#pragma unroll
  for (int q = 0; q < LP_SUMS; ++q) acc[q] = 0.0;
  int cnt = 0;
  for (int m = (int)threadIdx.x; m < n; m += LP_THREADS) {
    const uint32_t slot = s.slot[m] & ~PB_ACTIVE;
    double za[3], zb[3], A[6], B[3][6], C[21], gp[3], gt[6], L[6], e2;
    const double p[3] = {pts[3 * (size_t)slot], pts[3 * (size_t)slot + 1], pts[3 * (size_t)slot + 2]};
    bool front;
    pb_observations<Q8>(s, m, W, za, zb);
    pb_blocks(T, p, za, zb, c, w, e2, front, A, B, C, gp, gt);
    const bool active = front && e2 <= w.gate2 && pb_chol3(A, L);
    s.slot[m] = active ? slot | PB_ACTIVE : slot;
    if (!active) continue;
    cnt += 1;
    double Y[3][6], yp[3];
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) pb_solve3(L, B[0][cc], B[1][cc], B[2][cc], Y[0][cc], Y[1][cc], Y[2][cc]);
    pb_solve3(L, gp[0], gp[1], gp[2], yp[0], yp[1], yp[2]);
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int cc = r; cc < 6; ++cc) {
        acc[q] += C[q] - ((B[0][r] * Y[0][cc] + B[1][r] * Y[1][cc]) + B[2][r] * Y[2][cc]);
        ++q;
      }
      acc[21 + r] += gt[r] - ((B[0][r] * yp[0] + B[1][r] * yp[1]) + B[2][r] * yp[2]);
    }
    acc[27] += e2;
  }
  return lp_reduce(acc, cnt, s_red, s_cnt);
}

// The back-substitution of the points the last pass found active: p <- p - A^-1 (gp - B delta), the blocks recomputed
// under the model T that pass ran with.
template <bool Q8>
__device__ __forceinline__ void pb_backsub(const PbLds& s, int n, uint32_t W, const LpCam& c, const PbWeights& w,
                                           const double (&T)[12], const double (&delta)[6], double* pts) {
  for (int m = (int)threadIdx.x; m < n; m += LP_THREADS) {
    const uint32_t word = s.slot[m];
    if (!(word & PB_ACTIVE)) continue;                    // an inactive point keeps its p
    const size_t o = 3 * (size_t)(word & ~PB_ACTIVE);
    double za[3], zb[3], A[6], B[3][6], C[21], gp[3], gt[6], L[6], e2, rhs[3], dp[3];
    const double p[3] = {pts[o], pts[o + 1], pts[o + 2]};
    bool front;
    pb_observations<Q8>(s, m, W, za, zb);
    pb_blocks(T, p, za, zb, c, w, e2, front, A, B, C, gp, gt);
    pb_chol3(A, L);                                       // the same bits as in the pass that set PB_ACTIVE: it succeeds
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double bd = B[r][0] * delta[0];
#pragma unroll
      for (int cc = 1; cc < 6; ++cc) bd += B[r][cc] * delta[cc];
      rhs[r] = gp[r] - bd;
    }
    pb_solve3(L, rhs[0], rhs[1], rhs[2], dp[0], dp[1], dp[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) pts[o + r] = p[r] - dp[r];
  }
}

// One workgroup per pair.  match_in and out may be the same buffer: slot i is read and written by one thread at a time
// (the thread that examines it in the compaction, later the owner of its candidate), and only this workgroup touches row c.
template <bool Q8>
__global__ __launch_bounds__(LP_THREADS) void stereo_pair_bundle_kernel(
    const int32_t* match_in, const int* __restrict__ pair_a, const int* __restrict__ pair_b,
    const int32_t* __restrict__ stereo_idx, const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count,
    const int32_t* __restrict__ disp_q8, const double* __restrict__ T_in, const int32_t* __restrict__ info_in, int n_frames,
    int max_kp, uint32_t W, LpCam cam, PbWeights wgt, int iters, double* __restrict__ T_ab, double* __restrict__ S,
    double* __restrict__ chi2, double* __restrict__ points, int32_t* out, int32_t* __restrict__ info) {
  extern __shared__ uint32_t s_pb[];
  __shared__ double s_red[LP_WAVES * LP_SUMS];
  __shared__ double s_T[12];
  __shared__ double s_delta[6];
  __shared__ int s_w[LP_WAVES];
  __shared__ int s_fail;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = pair_a[c], b = pair_b[c];
  const bool passed = info_in[6 * c + 4] != 0;
  const LpPair p = lp_pair<Q8>(match_in, c, a, b, stereo_idx, kp_keys, kp_count, disp_q8, n_frames, max_kp);
  PbLds s;
  s.k1 = s_pb;
  s.k2 = s.k1 + max_kp;
  s.d1 = reinterpret_cast<int*>(s.k2 + max_kp);
  s.d2 = s.d1 + max_kp;
  s.slot = reinterpret_cast<uint32_t*>(s.d2 + max_kp);
  double* pts = points + (size_t)c * max_kp * 3;
  int32_t* row = out + (size_t)c * max_kp;

  // compaction in index order over every slot of the row: a candidate goes to LDS; every other slot gets its final
  // outputs here
  int n = 0;
  for (int i0 = 0; i0 < max_kp; i0 += LP_THREADS) {
    const int i = i0 + tid;
    LpCand cd;
    const bool valid = !passed && lp_candidate<Q8>(p, i, W, cam, cd);      // false for i >= nla, and nla <= max_kp
    const unsigned long long mask = __ballot(valid);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < LP_WAVES; ++w) {
      const int cw = s_w[w];
      before += w < wave ? cw : 0;
      total += cw;
    }
    if (valid) {
      const int pos = n + before + __popcll(mask & ((1ull << lane) - 1ull));      // <= its slot i < max_kp
      s.k1[pos] = cd.p1; s.k2[pos] = cd.p2; s.d1[pos] = cd.d1; s.d2[pos] = cd.d2; s.slot[pos] = (uint32_t)i;
    }
    if (i < max_kp && !valid) {
      row[i] = -1;
      pts[3 * (size_t)i] = 0.0;
      pts[3 * (size_t)i + 1] = 0.0;
      pts[3 * (size_t)i + 2] = 0.0;
    }
    n += total;
    __syncthreads();
  }

  double T[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) T[q] = T_in[(size_t)c * 12 + q];
  int status = passed ? 4 : (n < 3 ? 1 : 0), rounds = 0, n_first = 0, n_act = 0;

  if (status == 0) {                   // everything below is uniform over the block
    for (int m = tid; m < n; m += LP_THREADS) {      // p starts at the triangulation of za; from here on `points` is
      double za[3], zb[3], P[3];                     // read and written by the owner of the candidate alone
      pb_observations<Q8>(s, m, W, za, zb);
      lp_point(za[0], za[1], za[2], cam, P[0], P[1], P[2]);
      const size_t o = 3 * (size_t)s.slot[m];
#pragma unroll
      for (int r = 0; r < 3; ++r) pts[o + r] = P[r];
    }
    for (int it = 0;; ++it) {
      n_act = pb_accumulate<Q8>(s, n, W, cam, wgt, T, pts, s_red, s_w);
      if (it == 0) n_first = n_act;
      if (it == iters) break;
      if (n_act < 3) {                 // fewer than three points do not fix a pose: S is singular whatever its rounding says
        status = 3;
        break;
      }
      if (tid == 0) {
        double hh[21], g[6], x[6];
#pragma unroll
        for (int q = 0; q < 21; ++q) hh[q] = lp_total(s_red, q);
#pragma unroll
        for (int q = 0; q < 6; ++q) g[q] = lp_total(s_red, 21 + q);
        const bool ok = lp_solve6(hh, g, x);
        s_fail = ok ? 0 : 1;
        if (ok) {
          double xi[6], Tn[12];
#pragma unroll
          for (int q = 0; q < 6; ++q) {
            xi[q] = -x[q];
            s_delta[q] = x[q];
          }
          pose_retract(T, xi, Tn);
#pragma unroll
          for (int q = 0; q < 12; ++q) s_T[q] = Tn[q];
        }
      }
      __syncthreads();
      if (s_fail) {
        status = 3;
        break;
      }
      double delta[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) delta[q] = s_delta[q];
      pb_backsub<Q8>(s, n, W, cam, wgt, T, delta, pts);
#pragma unroll
      for (int q = 0; q < 12; ++q) T[q] = s_T[q];
      rounds += 1;
    }
  }

  // the candidates' slots, by their owners: an active point of a good pair keeps its match and its position
  for (int m = tid; m < n; m += LP_THREADS) {
    const uint32_t word = s.slot[m], i = word & ~PB_ACTIVE;
    const bool keep = status == 0 && (word & PB_ACTIVE) != 0;
    const int j = p.mt[i];             // read before the write below: the two rows may be one
    row[i] = keep ? j : -1;
    if (!keep) {
      pts[3 * (size_t)i] = 0.0;
      pts[3 * (size_t)i + 1] = 0.0;
      pts[3 * (size_t)i + 2] = 0.0;
    }
  }
  if (tid == 0) {
    int q = 0;
    for (int pp = 0; pp < 6; ++pp)
      for (int r = pp; r < 6; ++r) {
        const double v = status == 0 ? lp_total(s_red, q) : 0.0;
        ++q;
        S[(size_t)c * 36 + 6 * pp + r] = v;
        S[(size_t)c * 36 + 6 * r + pp] = v;
      }
    chi2[c] = status == 0 ? lp_total(s_red, 27) : 0.0;
    for (int k = 0; k < 12; ++k) T_ab[(size_t)c * 12 + k] = T[k];
    info[6 * c + 0] = n;
    info[6 * c + 1] = n_first;
    info[6 * c + 2] = status == 0 ? n_act : 0;
    info[6 * c + 3] = status;
    info[6 * c + 4] = rounds;
    info[6 * c + 5] = 0;
  }
}

}  // namespace

extern "C" int vus_stereo_pair_bundle(const int32_t* match_in, const int* pair_a, const int* pair_b, const int32_t* stereo_idx,
                                      const uint32_t* kp_keys, const int* kp_count, int n_frames, int n_pairs, int max_kp, int H,
                                      int W, const double* cam, const int32_t* disp_q8, const double* T_in,
                                      const int32_t* info_in, double sigma_uv_px, double sigma_disp_px, double gate, int iters,
                                      double* T_ab, double* S, double* chi2, double* points, int32_t* match_idx_out,
                                      int32_t* info, void* stream) {
  VUS_REQUIRE(match_in && pair_a && pair_b && stereo_idx && kp_keys && kp_count && cam && T_in && info_in && T_ab && S && chi2 &&
                  points && match_idx_out && info,
              "stereo_pair_bundle: null buffer");
  VUS_REQUIRE(n_pairs >= 1, "stereo_pair_bundle: n_pairs=%d, needs at least one pair", n_pairs);
  VUS_REQUIRE(n_frames >= 1, "stereo_pair_bundle: n_frames=%d, needs at least one frame", n_frames);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= VUS_LOOP_MAX_KP, "stereo_pair_bundle: max_kp=%d outside 1..%d", max_kp, VUS_LOOP_MAX_KP);
  VUS_REQUIRE(iters >= 0 && iters <= VUS_LOOP_MAX_REFINE, "stereo_pair_bundle: iters=%d outside 0..%d", iters,
              VUS_LOOP_MAX_REFINE);
  VUS_REQUIRE(H >= 1 && W >= 1, "stereo_pair_bundle: H=%d W=%d", H, W);
  VUS_REQUIRE(std::isfinite(sigma_uv_px) && sigma_uv_px > 0.0, "stereo_pair_bundle: sigma_uv_px=%g is not a positive number",
              sigma_uv_px);
  VUS_REQUIRE(std::isfinite(sigma_disp_px) && sigma_disp_px > 0.0, "stereo_pair_bundle: sigma_disp_px=%g is not a positive number",
              sigma_disp_px);
  VUS_REQUIRE(std::isfinite(gate) && gate > 0.0, "stereo_pair_bundle: gate=%g is not a positive number", gate);
  const double fx = cam[0], fy = cam[1], baseline = cam[4];
  VUS_REQUIRE(std::isfinite(fx) && fx > 0.0 && std::isfinite(fy) && fy > 0.0,
              "stereo_pair_bundle: focal lengths fx=%g fy=%g are not positive numbers", fx, fy);
  VUS_REQUIRE(std::isfinite(baseline) && baseline > 0.0, "stereo_pair_bundle: baseline=%g is not a positive number", baseline);
  const LpCam c = {fx, fy, cam[2], cam[3], fx * baseline, 0.0};
  const PbWeights w = {1.0 / (sigma_uv_px * sigma_uv_px), 1.0 / (sigma_disp_px * sigma_disp_px), gate * gate};
  // LDS: 20 B per keypoint slot next to 1.1 KiB of static LDS: 40,000 B at max_kp = 2000, 81,920 B at 4096
  const size_t lds = (size_t)max_kp * PB_LDS_PER_SLOT;
  auto* kernel = disp_q8 ? stereo_pair_bundle_kernel<true> : stereo_pair_bundle_kernel<false>;
  if (lds > 48 * 1024)
    VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
  kernel<<<n_pairs, LP_THREADS, lds, vus::as_stream(stream)>>>(match_in, pair_a, pair_b, stereo_idx, kp_keys, kp_count, disp_q8,
                                                              T_in, info_in, n_frames, max_kp, (uint32_t)W, c, w, iters, T_ab, S,
                                                              chi2, points, match_idx_out, info);
  VUS_CHECK_LAUNCH("stereo_pair_bundle");
  return VUS_OK;
}
