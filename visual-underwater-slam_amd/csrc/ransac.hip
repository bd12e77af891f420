// ransac.hip -- vus_two_point_ransac (include/vus_ransac.h): two-point RANSAC with a known inter-frame rotation on the
// left(t) -> left(t+1) matches, between the track matcher and vus_track_ids.
//
// Built with FRONTEND_FLAGS (-ffp-contract=off): every fp64 statement below is the header's, operation by operation, and
// must round like the numpy restatement of the test suite.  Do not fuse, reorder or "simplify" them.
#include "vus_common.h"
#include <cmath>
#include "../../include/vus_ransac.h"

namespace {

constexpr int RSC_THREADS = 256;                 // one lane per hypothesis at the default n_hyp
constexpr int RSC_WAVES = RSC_THREADS / 64;
constexpr int RSC_LDS_PER_MATCH = 5 * (int)sizeof(double);   // X, Y, Z, a2, b2 (+ one `static` bit)
constexpr int RSC_LDS_PER_PACKED = 2 * (int)sizeof(uint32_t);

struct RscCam {
  double fx, fy, cx, cy, tn2;
};

struct RscMatch {
  double X, Y, Z, a2, b2;
  bool stat;
};

__device__ __forceinline__ uint32_t rsc_mix(uint32_t x) {   // lowbias32
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// per-match values from the two key positions (y * W + x), as vus_track_ids decodes them
__device__ __forceinline__ RscMatch rsc_match(uint32_t p1, uint32_t p2, uint32_t W, const RscCam& c, const double (&r)[9]) {
  const uint32_t y1 = p1 / W, x1 = p1 - y1 * W, y2 = p2 / W, x2 = p2 - y2 * W;
  const double a1 = ((double)x1 - c.cx) / c.fx, b1 = ((double)y1 - c.cy) / c.fy;
  RscMatch m;
  m.a2 = ((double)x2 - c.cx) / c.fx;
  m.b2 = ((double)y2 - c.cy) / c.fy;
  m.X = (r[0] * a1 + r[1] * b1) + r[2];
  m.Y = (r[3] * a1 + r[4] * b1) + r[5];
  m.Z = (r[6] * a1 + r[7] * b1) + r[8];
  const double dx = m.a2 * m.Z - m.X, dy = m.b2 * m.Z - m.Y;
  m.stat = m.Z > 0.0 && (dx * dx + dy * dy) <= c.tn2 * (m.Z * m.Z);
  return m;
}

// m = p1 x p2 of a match
__device__ __forceinline__ void rsc_line(const RscMatch& a, double& mx, double& my, double& mz) {
  mx = a.Y - a.Z * a.b2;
  my = a.Z * a.a2 - a.X;
  mz = a.X * a.b2 - a.Y * a.a2;
}

__device__ __forceinline__ bool rsc_inlier(double tx, double ty, double tz, double X, double Y, double Z, double a2,
                                           double b2, bool stat, double tn2) {
  const double lx = ty * Z - tz * Y, ly = tz * X - tx * Z, lz = tx * Y - ty * X;
  const double e = (lx * a2 + ly * b2) + lz, q = lx * lx + ly * ly;
  return Z > 0.0 && (stat || (q > 0.0 && e * e <= tn2 * q));
}

// the pair's compacted matches in LDS: either the per-match values (RES) or the packed positions they are recomputed from
struct RscLds {
  double *X, *Y, *Z, *a2, *b2;
  uint32_t* stat;      // one bit per match
  uint2* packed;
};

template <bool RES>
__device__ __forceinline__ RscMatch rsc_load(const RscLds& s, int k, uint32_t W, const RscCam& c, const double (&r)[9]) {
  if (RES) {
    RscMatch m;
    m.X = s.X[k]; m.Y = s.Y[k]; m.Z = s.Z[k]; m.a2 = s.a2[k]; m.b2 = s.b2[k];
    m.stat = (s.stat[k >> 5] >> (k & 31)) & 1u;
    return m;
  }
  const uint2 q = s.packed[k];
  return rsc_match(q.x, q.y, W, c, r);
}

// t = m_i x m_j of hypothesis k; false if a sample is not in front of the second camera
template <bool RES>
__device__ __forceinline__ bool rsc_model(const RscLds& s, int n, uint32_t a, int k, uint32_t W, const RscCam& c,
                                          const double (&r)[9], double& tx, double& ty, double& tz) {
  const uint32_t r1 = rsc_mix(a ^ (uint32_t)(2 * k)), r2 = rsc_mix(a ^ (uint32_t)(2 * k + 1));
  const uint32_t i = r1 % (uint32_t)n, j = (i + 1u + r2 % (uint32_t)(n - 1)) % (uint32_t)n;
  const RscMatch A = rsc_load<RES>(s, (int)i, W, c, r), B = rsc_load<RES>(s, (int)j, W, c, r);
  double ax, ay, az, bx, by, bz;
  rsc_line(A, ax, ay, az);
  rsc_line(B, bx, by, bz);
  tx = ay * bz - az * by;
  ty = az * bx - ax * bz;
  tz = ax * by - ay * bx;
  return A.Z > 0.0 && B.Z > 0.0;
}

// the best (count, lowest k) of this lane's hypotheses k = tid, tid + RSC_THREADS, ... as ((count + 1) << 12) | (4095 - k)
template <bool RES>
__device__ __forceinline__ uint32_t rsc_hypotheses(const RscLds& s, int n, int n_hyp, uint32_t a, uint32_t W,
                                                   const RscCam& c, const double (&r)[9]) {
  uint32_t best = 0;
  for (int k = (int)threadIdx.x; k < n_hyp; k += RSC_THREADS) {
    double tx, ty, tz;
    int cnt = -1;
    if (rsc_model<RES>(s, n, a, k, W, c, r, tx, ty, tz)) {
      cnt = 0;
      if (RES) {
        // every lane reads the same address: a broadcast, no bank conflict; 32 matches share one word of `static` bits
        for (int k0 = 0; k0 < n; k0 += 32) {
          const uint32_t bits = s.stat[k0 >> 5];
          const int m1 = min(32, n - k0);
#pragma unroll 4
          for (int u = 0; u < m1; ++u) {
            const int m = k0 + u;
            cnt += rsc_inlier(tx, ty, tz, s.X[m], s.Y[m], s.Z[m], s.a2[m], s.b2[m], (bits >> u) & 1u, c.tn2) ? 1 : 0;
          }
        }
      } else {
        for (int m = 0; m < n; ++m) {
          const RscMatch M = rsc_load<false>(s, m, W, c, r);
          cnt += rsc_inlier(tx, ty, tz, M.X, M.Y, M.Z, M.a2, M.b2, M.stat, c.tn2) ? 1 : 0;
        }
      }
    }
    const uint32_t key = ((uint32_t)(cnt + 1) << 12) | (uint32_t)(VUS_RANSAC_MAX_HYP - 1 - k);
    best = max(best, key);       // k ascends: an equal count of a later k has the smaller key
  }
  return best;
}

__device__ __forceinline__ int rsc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the workgroup, returned to every thread; s_w: RSC_WAVES ints, reusable after the call
__device__ __forceinline__ int rsc_block_sum(int v, int* s_w) {
  v = rsc_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < RSC_WAVES; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

// One workgroup per frame pair.  track_idx and out may be the same buffer: a thread reads slot i before it writes it, and
// only this workgroup touches row p.
__global__ __launch_bounds__(RSC_THREADS) void two_point_ransac_kernel(
    const int32_t* track_idx, const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count, int max_kp,
    uint32_t W, const double* __restrict__ rot, RscCam cam, int n_hyp, uint32_t seed, int lds_matches, int32_t* out,
    int32_t* __restrict__ info) {
  extern __shared__ double s_rsc[];
  __shared__ int s_w[RSC_WAVES];
  __shared__ uint32_t s_key[RSC_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nl = min(kp_count[2 * p], max_kp), nn = min(kp_count[2 * p + 2], max_kp);   // a negative count: no keypoint
  const int32_t* trk = track_idx + (size_t)p * max_kp;
  const uint32_t* k1 = kp_keys + (size_t)(2 * p) * max_kp;
  const uint32_t* k2 = kp_keys + (size_t)(2 * p + 2) * max_kp;
  double r[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) r[u] = rot[(size_t)p * 9 + u];

  // n first: it decides where the per-match values live
  int local = 0;
  for (int i = tid; i < nl; i += RSC_THREADS) {
    const int j = trk[i];
    local += (j >= 0 && j < nn) ? 1 : 0;
  }
  const int n = rsc_block_sum(local, s_w);
  const bool resident = n <= lds_matches;
  RscLds s;
  s.X = s_rsc;
  s.Y = s.X + lds_matches;
  s.Z = s.Y + lds_matches;
  s.a2 = s.Z + lds_matches;
  s.b2 = s.a2 + lds_matches;
  s.stat = reinterpret_cast<uint32_t*>(s.b2 + lds_matches);
  s.packed = reinterpret_cast<uint2*>(s_rsc);
  if (resident)
    for (int w = tid; w < (n + 31) / 32; w += RSC_THREADS) s.stat[w] = 0u;
  __syncthreads();

  // compaction in index order: a ballot per wave, the waves' totals through LDS
  int base = 0;
  for (int i0 = 0; i0 < nl; i0 += RSC_THREADS) {
    const int i = i0 + tid;
    const int j = i < nl ? trk[i] : -1;
    const bool valid = j >= 0 && j < nn;
    const unsigned long long mask = __ballot(valid);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RSC_WAVES; ++w) {
      const int c = s_w[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (valid) {
      const int pos = base + before + __popcll(mask & ((1ull << lane) - 1ull));     // < n by construction
      const uint32_t p1 = k1[i] & VUS_KEY_POS_MASK, p2 = k2[j] & VUS_KEY_POS_MASK;
      if (resident) {
        const RscMatch m = rsc_match(p1, p2, W, cam, r);
        s.X[pos] = m.X; s.Y[pos] = m.Y; s.Z[pos] = m.Z; s.a2[pos] = m.a2; s.b2[pos] = m.b2;
        if (m.stat) atomicOr(&s.stat[pos >> 5], 1u << (pos & 31));
      } else {
        s.packed[pos] = make_uint2(p1, p2);
      }
    }
    base += total;
    __syncthreads();
  }

  // hypotheses
  const uint32_t a = rsc_mix(seed + 0x9E3779B9u * (uint32_t)(p + 1));
  uint32_t key = 0;
  if (n >= 2) key = resident ? rsc_hypotheses<true>(s, n, n_hyp, a, W, cam, r) : rsc_hypotheses<false>(s, n, n_hyp, a, W, cam, r);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o));
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < RSC_WAVES; ++w) key = max(key, s_key[w]);
  int best = -1;
  double tx = 0.0, ty = 0.0, tz = 0.0;
  if ((int)(key >> 12) - 1 >= 0) {       // n >= 2 and some hypothesis had both samples in front
    best = VUS_RANSAC_MAX_HYP - 1 - (int)(key & 4095u);
    if (resident) rsc_model<true>(s, n, a, best, W, cam, r, tx, ty, tz);
    else rsc_model<false>(s, n, a, best, W, cam, r, tx, ty, tz);
  }

  // the output row: every slot, the per-match values recomputed from the keys (the same operations as above)
  int n_surv = 0, n_stat = 0;
  for (int i = tid; i < max_kp; i += RSC_THREADS) {
    int o = -1;
    if (i < nl) {
      const int j = trk[i];
      if (j >= 0 && j < nn) {
        const RscMatch m = rsc_match(k1[i] & VUS_KEY_POS_MASK, k2[j] & VUS_KEY_POS_MASK, W, cam, r);
        const bool keep = best < 0 ? m.Z > 0.0 : rsc_inlier(tx, ty, tz, m.X, m.Y, m.Z, m.a2, m.b2, m.stat, cam.tn2);
        if (keep) o = j;
        n_surv += keep ? 1 : 0;
        n_stat += m.stat ? 1 : 0;
      }
    }
    out[(size_t)p * max_kp + i] = o;
  }
  n_surv = rsc_block_sum(n_surv, s_w);
  n_stat = rsc_block_sum(n_stat, s_w);
  if (tid == 0) {
    info[4 * p + 0] = n;
    info[4 * p + 1] = n_surv;
    info[4 * p + 2] = best;
    info[4 * p + 3] = n_stat;
  }
}

}  // namespace

extern "C" int vus_two_point_ransac(const int32_t* track_idx, const uint32_t* kp_keys, const int* kp_count, int n_frames,
                                    int max_kp, int H, int W, const double* rot, const double* cam, double threshold_px,
                                    int n_hyp, uint32_t seed, int32_t* track_idx_out, int32_t* info, void* stream) {
  VUS_REQUIRE(track_idx && kp_keys && kp_count && rot && cam && track_idx_out && info, "null buffer");
  VUS_REQUIRE(n_frames >= 2, "two_point_ransac: n_frames=%d, needs at least one frame pair", n_frames);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= VUS_RANSAC_MAX_KP, "two_point_ransac: max_kp=%d outside 1..%d", max_kp,
              VUS_RANSAC_MAX_KP);
  VUS_REQUIRE(n_hyp >= 1 && n_hyp <= VUS_RANSAC_MAX_HYP, "two_point_ransac: n_hyp=%d outside 1..%d", n_hyp,
              VUS_RANSAC_MAX_HYP);
  VUS_REQUIRE(H >= 1 && W >= 1, "two_point_ransac: H=%d W=%d", H, W);
  VUS_REQUIRE(std::isfinite(threshold_px) && threshold_px > 0.0, "two_point_ransac: threshold_px=%g is not a positive number",
              threshold_px);
  const double fx = cam[0], fy = cam[1];
  VUS_REQUIRE(std::isfinite(fx) && fx > 0.0 && std::isfinite(fy) && fy > 0.0,
              "two_point_ransac: focal lengths fx=%g fy=%g are not positive numbers", fx, fy);
  const double tn = threshold_px / ((fx + fy) / 2.0);
  const RscCam c = {fx, fy, cam[2], cam[3], tn * tn};
  // LDS: the per-match values of up to VUS_RANSAC_LDS_MATCHES matches (40 B each + one bit), or -- where max_kp admits
  // more matches than that -- 8 B of packed positions per match, whichever is larger: 80,252 B at max_kp >= 2000, next to
  // 32 B of static LDS, so two workgroups share a CU's 160 KiB
  const int lds_matches = max_kp < VUS_RANSAC_LDS_MATCHES ? max_kp : VUS_RANSAC_LDS_MATCHES;
  size_t lds = (size_t)lds_matches * RSC_LDS_PER_MATCH + (size_t)((lds_matches + 31) / 32) * sizeof(uint32_t);
  if (max_kp > lds_matches && (size_t)max_kp * RSC_LDS_PER_PACKED > lds) lds = (size_t)max_kp * RSC_LDS_PER_PACKED;
  if (lds > 48 * 1024)
    VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(two_point_ransac_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  two_point_ransac_kernel<<<n_frames - 1, RSC_THREADS, lds, vus::as_stream(stream)>>>(
      track_idx, kp_keys, kp_count, max_kp, (uint32_t)W, rot, c, n_hyp, seed, lds_matches, track_idx_out, info);
  VUS_CHECK_LAUNCH("two_point_ransac");
  return VUS_OK;
}
