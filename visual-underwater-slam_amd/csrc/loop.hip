// loop.hip -- vus_stereo_pair_pose and vus_stereo_pair_pose_q8 (include/vus_loop.h): the relative pose of two stereo
// keyframes by three-point RANSAC on their triangulated matches and a Gauss-Newton refit of the left-image reprojection
// error.  One kernel text, instantiated twice: Q8 = false takes the integer disparities of the keys (the instantiation the
// first entry point has always launched), Q8 = true the refined ones of vus_stereo_refine, in 1/256 px.
//
// Built with FRONTEND_FLAGS (-ffp-contract=off): every fp64 statement below is the header's, operation by operation, as
// the numpy restatement of the test suite (tests/loop_ref.py) writes it.  Do not fuse, reorder or "simplify" them.
#include "vus_common.h"
#include <cmath>
#include "se3_device.h"
#include "loop_device.h"   // the candidate rule, the reduction tree and the 6 x 6 solve, shared with pair_bundle.hip
#include "../../include/vus_loop.h"

namespace {

constexpr int LP_LDS_PER_SLOT = 3 * (int)sizeof(double) + 2 * (int)sizeof(float) + (int)sizeof(int);   // P, (u, v), d2

// the pair's compacted candidates in LDS
struct LpLds {
  double *Px, *Py, *Pz;
  float *u, *v;
  int* d2;
};

__device__ __forceinline__ uint32_t lp_mix(uint32_t x) {   // lowbias32
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// the orthonormal triad of a sample, e[0..2] = e1, e[3..5] = e2, e[6..8] = e3; false if degenerate
__device__ __forceinline__ bool lp_triad(const double (&A)[3], const double (&B)[3], const double (&C)[3], double (&e)[9]) {
  double e1[3], f[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    e1[r] = B[r] - A[r];
    f[r] = C[r] - A[r];
  }
  const double c3[3] = {e1[1] * f[2] - e1[2] * f[1], e1[2] * f[0] - e1[0] * f[2], e1[0] * f[1] - e1[1] * f[0]};
  const double n1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
  const double n2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
  const double n3 = (c3[0] * c3[0] + c3[1] * c3[1]) + c3[2] * c3[2];
  if (!(n3 > 1e-6 * (n1 * n2))) return false;
  const double s1 = sqrt(n1), s3 = sqrt(n3);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    e[r] = e1[r] / s1;
    e[6 + r] = c3[r] / s3;
  }
  e[3] = e[7] * e[2] - e[8] * e[1];
  e[4] = e[8] * e[0] - e[6] * e[2];
  e[5] = e[6] * e[1] - e[7] * e[0];
  return true;
}

// T (flat12) of hypothesis k; false for a degenerate sample.  n >= 3.
template <bool Q8>
__device__ __forceinline__ bool lp_model(const LpLds& s, int n, uint32_t h, int k, const LpCam& c, double (&T)[12]) {
  const uint32_t r1 = lp_mix(h ^ (uint32_t)(3 * k)), r2 = lp_mix(h ^ (uint32_t)(3 * k + 1)), r3 = lp_mix(h ^ (uint32_t)(3 * k + 2));
  const uint32_t i = r1 % (uint32_t)n, j = (i + 1u + r2 % (uint32_t)(n - 1)) % (uint32_t)n;
  uint32_t l = r3 % (uint32_t)(n - 2);
  if (l >= min(i, j)) l += 1u;
  if (l >= max(i, j)) l += 1u;               // i, j, l distinct and below n
  const uint32_t idx[3] = {i, j, l};
  double P[3][3], Q[3][3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint32_t m = idx[q];
    P[q][0] = s.Px[m]; P[q][1] = s.Py[m]; P[q][2] = s.Pz[m];
    lp_point((double)s.u[m], (double)s.v[m], lp_disparity<Q8>(s.d2[m]), c, Q[q][0], Q[q][1], Q[q][2]);
  }
  double F[9], E[9];
  const bool okp = lp_triad(P[0], P[1], P[2], F);
  const bool okq = lp_triad(Q[0], Q[1], Q[2], E);
  if (!(okp && okq)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) T[3 * r + cc] = (F[r] * E[cc] + F[3 + r] * E[3 + cc]) + F[6 + r] * E[6 + cc];
#pragma unroll
  for (int r = 0; r < 3; ++r) T[9 + r] = P[0][r] - ((T[3 * r] * Q[0][0] + T[3 * r + 1] * Q[0][1]) + T[3 * r + 2] * Q[0][2]);
  return true;
}

// X = R^T (P - t) and the inlier test
__device__ __forceinline__ bool lp_inlier(const double (&T)[12], double Px, double Py, double Pz, double u, double v,
                                          const LpCam& c, double (&X)[3]) {
  const double Dx = Px - T[9], Dy = Py - T[10], Dz = Pz - T[11];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) X[cc] = (T[cc] * Dx + T[3 + cc] * Dy) + T[6 + cc] * Dz;
  const double ex = c.fx * X[0] - (u - c.cx) * X[2], ey = c.fy * X[1] - (v - c.cy) * X[2];
  return X[2] > 0.0 && (ex * ex + ey * ey) <= c.thr2 * (X[2] * X[2]);
}

// the best (count, lowest k) of this lane's hypotheses k = tid, tid + LP_THREADS, ... as ((count + 1) << 12) | (4095 - k)
template <bool Q8>
__device__ __forceinline__ uint32_t lp_hypotheses(const LpLds& s, int n, int n_hyp, uint32_t h, const LpCam& c) {
  uint32_t best = 0;
  for (int k = (int)threadIdx.x; k < n_hyp; k += LP_THREADS) {
    double T[12], X[3];
    int cnt = -1;
    if (lp_model<Q8>(s, n, h, k, c, T)) {
      cnt = 0;
#pragma unroll 4
      for (int m = 0; m < n; ++m)    // every lane reads the same address: a broadcast, no bank conflict
        cnt += lp_inlier(T, s.Px[m], s.Py[m], s.Pz[m], (double)s.u[m], (double)s.v[m], c, X) ? 1 : 0;
    }
    const uint32_t key = ((uint32_t)(cnt + 1) << 12) | (uint32_t)(VUS_LOOP_MAX_HYP - 1 - k);
    best = max(best, key);           // k ascends: an equal count of a later k has the smaller key
  }
  return best;
}

// One refit pass: H, g and rss over the inliers of T, left per wave in s_red [LP_WAVES][LP_SUMS] (the caller adds the waves
// in order); returns the number of inliers to every thread.  Ends with a barrier.
__device__ __forceinline__ int lp_accumulate(const LpLds& s, int n, const LpCam& c, const double (&T)[12], double* s_red,
                                             int* s_cnt) {
  double acc[LP_SUMS];
#pragma unroll
  for (int q = 0; q < LP_SUMS; ++q) acc[q] = 0.0;
  int cnt = 0;
  for (int m = (int)threadIdx.x; m < n; m += LP_THREADS) {
    const double u = (double)s.u[m], v = (double)s.v[m];
    double X[3];
    if (!lp_inlier(T, s.Px[m], s.Py[m], s.Pz[m], u, v, c, X)) continue;
    cnt += 1;
    const double iz = 1.0 / X[2], a = c.fx * iz, b = c.fy * iz, px = X[0] * iz, py = X[1] * iz;
    const double r0 = (c.fx * px + c.cx) - u, r1 = (c.fy * py + c.cy) - v;
    const double g2 = -(a * px), h2 = -(b * py);
    const double J0[6] = {-(g2 * X[1]), g2 * X[0] - a * X[2], a * X[1], -a, 0.0, -g2};
    const double J1[6] = {b * X[2] - h2 * X[1], h2 * X[0], -(b * X[0]), 0.0, -b, -h2};
    int q = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int r = p; r < 6; ++r) acc[q++] += J0[p] * J0[r] + J1[p] * J1[r];
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[21 + p] += J0[p] * r0 + J1[p] * r1;
    acc[27] += r0 * r0 + r1 * r1;
  }
  return lp_reduce(acc, cnt, s_red, s_cnt);
}

// One workgroup per pair.  match_idx and out may be the same buffer: a thread reads slot i before it writes it, and only
// this workgroup touches row c.  disp_q8 is read by the Q8 instantiation only.
template <bool Q8>
__global__ __launch_bounds__(LP_THREADS) void stereo_pair_pose_kernel(
    const int32_t* match_idx, const int* __restrict__ pair_a, const int* __restrict__ pair_b,
    const int32_t* __restrict__ stereo_idx, const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count,
    int n_frames, int max_kp, uint32_t W, LpCam cam, int n_hyp, uint32_t seed, int refine_iters, double* __restrict__ T_ab,
    double* __restrict__ JtJ, double* __restrict__ rss, int32_t* out, int32_t* __restrict__ info,
    const int32_t* __restrict__ disp_q8) {      // last: the arguments of the Q8 = false instantiation keep their offsets
  extern __shared__ double s_lp[];
  __shared__ double s_red[LP_WAVES * LP_SUMS];
  __shared__ double s_T[12];
  __shared__ int s_w[LP_WAVES];
  __shared__ uint32_t s_key[LP_WAVES];
  __shared__ int s_fail;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = pair_a[c], b = pair_b[c];
  const bool pair_ok = a >= 0 && a < n_frames && b >= 0 && b < n_frames && a != b;
  const int fa = pair_ok ? a : 0, fb = pair_ok ? b : 0;     // a refused pair indexes frame 0 and, with empty lists, reads nothing
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
  LpLds s;
  s.Px = s_lp;
  s.Py = s.Px + max_kp;
  s.Pz = s.Py + max_kp;
  s.u = reinterpret_cast<float*>(s.Pz + max_kp);
  s.v = s.u + max_kp;
  s.d2 = reinterpret_cast<int*>(s.v + max_kp);

  // compaction in index order: a ballot per wave, the waves' totals through LDS
  int n = 0;
  for (int i0 = 0; i0 < p.nla; i0 += LP_THREADS) {
    LpCand cd;
    const bool valid = lp_candidate<Q8>(p, i0 + tid, W, cam, cd);
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
      s.Px[pos] = cd.Px; s.Py[pos] = cd.Py; s.Pz[pos] = cd.Pz;
      s.u[pos] = cd.u; s.v[pos] = cd.v; s.d2[pos] = cd.d2;
    }
    n += total;
    __syncthreads();
  }

  // hypotheses
  const uint32_t h = lp_mix(seed + 0x9E3779B9u * (uint32_t)(c + 1));
  uint32_t key = 0;
  if (n >= 3) key = lp_hypotheses<Q8>(s, n, n_hyp, h, cam);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o));
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < LP_WAVES; ++w) key = max(key, s_key[w]);
  const int best_count = (int)(key >> 12) - 1;
  int best = -1, status = n < 3 ? 1 : 2, rounds = 0, n_in = 0;
  double T[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};

  if (best_count >= 0) {             // n >= 3 and some sample was not degenerate; everything below is uniform over the block
    best = VUS_LOOP_MAX_HYP - 1 - (int)(key & 4095u);
    lp_model<Q8>(s, n, h, best, cam, T);
    status = 0;
    for (int it = 0;; ++it) {
      n_in = lp_accumulate(s, n, cam, T, s_red, s_w);
      if (it == refine_iters) break;
      if (n_in < 3) {                // fewer than three points do not fix a pose: H is singular whatever its rounding says
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
          for (int q = 0; q < 6; ++q) xi[q] = -x[q];
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
#pragma unroll
      for (int q = 0; q < 12; ++q) T[q] = s_T[q];
      rounds += 1;
    }
  }

  // the output row: every slot, the candidate recomputed from the tables (the same operations as above)
  for (int i = tid; i < max_kp; i += LP_THREADS) {
    LpCand cd;
    double X[3];
    int o = -1;
    if (status == 0 && lp_candidate<Q8>(p, i, W, cam, cd) && lp_inlier(T, cd.Px, cd.Py, cd.Pz, (double)cd.u, (double)cd.v, cam, X))
      o = cd.j;
    out[(size_t)c * max_kp + i] = o;
  }
  if (tid == 0) {
    int q = 0;
    for (int pp = 0; pp < 6; ++pp)
      for (int r = pp; r < 6; ++r) {
        const double v = status == 0 ? lp_total(s_red, q) : 0.0;
        ++q;
        JtJ[(size_t)c * 36 + 6 * pp + r] = v;
        JtJ[(size_t)c * 36 + 6 * r + pp] = v;
      }
    rss[c] = status == 0 ? lp_total(s_red, 27) : 0.0;
    for (int k = 0; k < 12; ++k) T_ab[(size_t)c * 12 + k] = T[k];
    info[6 * c + 0] = n;
    info[6 * c + 1] = best;
    info[6 * c + 2] = best_count;
    info[6 * c + 3] = status == 0 ? n_in : 0;
    info[6 * c + 4] = status;
    info[6 * c + 5] = rounds;
  }
}

}  // namespace

namespace {

// both entry points: validation, then the instantiation that disp_q8 selects (null: integer disparities)
int lp_launch(const int32_t* match_idx, const int* pair_a, const int* pair_b, const int32_t* stereo_idx, const uint32_t* kp_keys,
              const int* kp_count, const int32_t* disp_q8, int n_frames, int n_pairs, int max_kp, int H, int W, const double* cam,
              double threshold_px, int n_hyp, uint32_t seed, int refine_iters, double* T_ab, double* JtJ, double* rss,
              int32_t* match_idx_out, int32_t* info, void* stream) {
  VUS_REQUIRE(match_idx && pair_a && pair_b && stereo_idx && kp_keys && kp_count && cam && T_ab && JtJ && rss &&
                  match_idx_out && info,
              "stereo_pair_pose: null buffer");
  VUS_REQUIRE(n_pairs >= 1, "stereo_pair_pose: n_pairs=%d, needs at least one pair", n_pairs);
  VUS_REQUIRE(n_frames >= 1, "stereo_pair_pose: n_frames=%d, needs at least one frame", n_frames);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= VUS_LOOP_MAX_KP, "stereo_pair_pose: max_kp=%d outside 1..%d", max_kp, VUS_LOOP_MAX_KP);
  VUS_REQUIRE(n_hyp >= 1 && n_hyp <= VUS_LOOP_MAX_HYP, "stereo_pair_pose: n_hyp=%d outside 1..%d", n_hyp, VUS_LOOP_MAX_HYP);
  VUS_REQUIRE(refine_iters >= 0 && refine_iters <= VUS_LOOP_MAX_REFINE, "stereo_pair_pose: refine_iters=%d outside 0..%d",
              refine_iters, VUS_LOOP_MAX_REFINE);
  VUS_REQUIRE(H >= 1 && W >= 1, "stereo_pair_pose: H=%d W=%d", H, W);
  VUS_REQUIRE(std::isfinite(threshold_px) && threshold_px > 0.0, "stereo_pair_pose: threshold_px=%g is not a positive number",
              threshold_px);
  const double fx = cam[0], fy = cam[1], baseline = cam[4];
  VUS_REQUIRE(std::isfinite(fx) && fx > 0.0 && std::isfinite(fy) && fy > 0.0,
              "stereo_pair_pose: focal lengths fx=%g fy=%g are not positive numbers", fx, fy);
  VUS_REQUIRE(std::isfinite(baseline) && baseline > 0.0, "stereo_pair_pose: baseline=%g is not a positive number", baseline);
  const LpCam c = {fx, fy, cam[2], cam[3], fx * baseline, threshold_px * threshold_px};
  // LDS: 36 B per keypoint slot (all candidates stay resident), next to 1 KiB of static LDS: 72,000 B at max_kp = 2000 (two
  // workgroups per CU), 147,456 B at 4096
  const size_t lds = (size_t)max_kp * LP_LDS_PER_SLOT;
  auto* kernel = disp_q8 ? stereo_pair_pose_kernel<true> : stereo_pair_pose_kernel<false>;
  if (lds > 48 * 1024)
    VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
  kernel<<<n_pairs, LP_THREADS, lds, vus::as_stream(stream)>>>(match_idx, pair_a, pair_b, stereo_idx, kp_keys, kp_count, n_frames,
                                                              max_kp, (uint32_t)W, c, n_hyp, seed, refine_iters, T_ab, JtJ, rss,
                                                              match_idx_out, info, disp_q8);
  VUS_CHECK_LAUNCH("stereo_pair_pose");
  return VUS_OK;
}

}  // namespace

extern "C" int vus_stereo_pair_pose(const int32_t* match_idx, const int* pair_a, const int* pair_b, const int32_t* stereo_idx,
                                    const uint32_t* kp_keys, const int* kp_count, int n_frames, int n_pairs, int max_kp, int H,
                                    int W, const double* cam, double threshold_px, int n_hyp, uint32_t seed, int refine_iters,
                                    double* T_ab, double* JtJ, double* rss, int32_t* match_idx_out, int32_t* info,
                                    void* stream) {
  return lp_launch(match_idx, pair_a, pair_b, stereo_idx, kp_keys, kp_count, nullptr, n_frames, n_pairs, max_kp, H, W, cam,
                   threshold_px, n_hyp, seed, refine_iters, T_ab, JtJ, rss, match_idx_out, info, stream);
}

extern "C" int vus_stereo_pair_pose_q8(const int32_t* match_idx, const int* pair_a, const int* pair_b,
                                       const int32_t* stereo_idx, const uint32_t* kp_keys, const int* kp_count, int n_frames,
                                       int n_pairs, int max_kp, int H, int W, const double* cam, double threshold_px, int n_hyp,
                                       uint32_t seed, int refine_iters, const int32_t* disp_q8, double* T_ab, double* JtJ,
                                       double* rss, int32_t* match_idx_out, int32_t* info, void* stream) {
  return lp_launch(match_idx, pair_a, pair_b, stereo_idx, kp_keys, kp_count, disp_q8, n_frames, n_pairs, max_kp, H, W, cam,
                   threshold_px, n_hyp, seed, refine_iters, T_ab, JtJ, rss, match_idx_out, info, stream);
}
