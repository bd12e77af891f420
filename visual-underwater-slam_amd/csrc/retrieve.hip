// retrieve.hip -- loop-closure candidates by appearance (include/vus_retrieval.h): for every ordered pair of keyframes the
// number of one keyframe's strongest descriptors that have a near neighbour among the other's.
//
// Design notes (MI355X):
//  * the all-pairs Hamming distances are the FP4 block-scaled GEMM of the track matcher (fp4_hamming.h; the structure of
//    hamming_match_mfma_kernel in match.hip): queries = B operand, expanded once into registers, KS_QWG per workgroup;
//    train descriptors = A operand, expanded per KS_CHUNK-row chunk into LDS and shared by the four waves, the next chunk's
//    words loaded while this one's tiles run; four MFMAs per 32x32 tile over K = 256.
//  * one workgroup keeps its query fragments and walks KS_TB consecutive train keyframes: the queries are 16 KB per
//    workgroup, the trains it meets 16 KB each, and the pipeline of chunk loads runs across the train boundaries.
//  * the epilogue needs no index: per column the maximum dot over every row of the train image, then one compare.
#include "frontend_common.h"
#include "fp4_hamming.h"
#include "../../include/vus_retrieval.h"
#include <algorithm>

namespace {

constexpr int KS_CHUNK = 128;                 // trains expanded per LDS chunk
constexpr int KS_QT = 4;                      // 32-query column tiles per wave
constexpr int KS_QWG = 4 * 32 * KS_QT;        // queries per workgroup
constexpr int KS_TB = VUS_RETRIEVAL_TRAIN_BLOCK;   // consecutive train keyframes per workgroup
constexpr int KS_ITEMS = KS_CHUNK * 8 / 256;  // (train, 32-bit word) items per thread and chunk
constexpr long long KS_MAX_GRID = 1ll << 22;  // workgroups per launch; work items past that are strided over

// descriptors of image m that take part: 0 for an image number outside [0, n_img), with which nothing is indexed
__device__ __forceinline__ int used_count(const int* __restrict__ kp_count, int n_img, int max_kp, int top, int m) {
  if (m < 0 || m >= n_img) return 0;
  return min(min(max(kp_count[m], 0), max_kp), top);
}

__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// max over the 16 values of this lane's rows and the running maximum
__device__ __forceinline__ float tile_max(const v16f_t& acc, float prev) {
  const float m0 = max3f(acc[0], acc[1], acc[2]), m1 = max3f(acc[3], acc[4], acc[5]), m2 = max3f(acc[6], acc[7], acc[8]),
              m3 = max3f(acc[9], acc[10], acc[11]), m4 = max3f(acc[12], acc[13], acc[14]), m5 = max3f(acc[15], prev, m0);
  return max3f(max3f(m1, m2, m3), m4, m5);
}

// this thread's items of the chunk of `nt` train descriptors at dt that starts at row t0; a row past nt loads row nt - 1,
// whose dots the epilogue masks
__device__ __forceinline__ void load_chunk(uint32_t (&xw)[KS_ITEMS], const uint32_t* __restrict__ dt, int t0, int nt, int tid) {
#pragma unroll
  for (int u = 0; u < KS_ITEMS; ++u) xw[u] = dt[(size_t)min(t0 + ((tid + 256 * u) >> 3), nt - 1) * 8 + (tid & 7)];
}

// A work item is (block of KS_TB train columns, query row q, block of KS_QWG queries), the query block fastest and the
// train block slowest.  Workgroups go to the eight XCDs round robin: with the train block fastest and a multiple of eight
// blocks per row, a triangular t_limit leaves XCD 0 half as many live items again as XCD 7 (1.22 instead of 0.81 ms at 256
// keyframes, profiles/loop_retrieval.md).  In this order every XCD gets the same share, and neighbouring workgroups share
// their trains in L2.
// waves_per_eu(3): 168 registers and 3 waves per SIMD, with two dwords of values that do not change inside the loops spilled
// before them and reloaded once per work item; without the hint 172 registers, 2 waves, no spill, and 7 % more time at 2000
// keyframes.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void keyframe_similarity_kernel(
    const uint32_t* __restrict__ desc32, const int* __restrict__ kp_count, int n_img, int max_kp,
    const int* __restrict__ q_img, int n_q, const int* __restrict__ t_img, int n_t, const int* __restrict__ t_limit, int top,
    float min_dot, int n_qb, long long n_work, int32_t* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) uint8_t s_t[KS_CHUNK * HM_ROWB];
  __shared__ uint32_t s_lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_lut[tid] = spread_fp4(tid);
  __syncthreads();
  const int r = lane & 31, h = lane >> 5;
  const v16f_t zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {      // every test up to the fragments is workgroup-uniform
    const int qb = (int)(w % n_qb);
    const long long wq = w / n_qb;
    const int q = (int)(wq % n_q), tb = (int)(wq / n_q);
    const int lim = t_limit ? clampi(t_limit[q], 0, n_t) : n_t;
    const int t_beg = tb * KS_TB, t_end = min(t_beg + KS_TB, lim);
    if (t_beg >= lim) continue;                                     // nothing of this block is asked for: S stays 0
    const int qi = q_img[q];
    const int nq = used_count(kp_count, n_img, max_kp, top, qi);
    if (qb * KS_QWG >= nq) continue;                                // a workgroup without queries
    const int wq0 = qb * KS_QWG + 32 * KS_QT * wave;                // first query of this wave
    const int q0 = wq0 + r;                                         // column tile c holds query q0 + 32 c
    const bool wave_busy = wq0 < nq;                                // a wave without queries only helps expand the trains
    // B fragments: MFMA ks, lane half h <-> descriptor word 2 ks + h; a column at or past nq is never counted
    v4i_t bq[KS_QT][4];
#pragma unroll
    for (int c = 0; c < KS_QT; ++c) {
      const uint32_t* dq = desc32 + ((size_t)qi * max_kp + min(q0 + 32 * c, max_kp - 1)) * 8 + h;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bq[c][ks] = spread_word(s_lut, dq[2 * ks]);
    }
    uint32_t xw[KS_ITEMS];            // the chunk (pre_t, pre_t0), loaded one chunk ahead -- across train boundaries too
    int pre_t = -1, pre_t0 = 0;
    for (int t = t_beg; t < t_end; ++t) {
      const int ti = t_img[t];
      const int nt = used_count(kp_count, n_img, max_kp, top, ti);
      const uint32_t* dt = desc32 + (size_t)(nt > 0 ? ti : 0) * max_kp * 8;
      float cm[KS_QT];                // per column: the largest dot over this lane's rows of train image t
#pragma unroll
      for (int c = 0; c < KS_QT; ++c) cm[c] = -INFINITY;
      for (int t0 = 0; t0 < nt; t0 += KS_CHUNK) {
        if (pre_t != t || pre_t0 != t0) load_chunk(xw, dt, t0, nt, tid);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < KS_ITEMS; ++u) {
          const int item = tid + 256 * u;
          *reinterpret_cast<v4i_t*>(s_t + (item >> 3) * HM_ROWB + 16 * (item & 7)) = spread_word(s_lut, xw[u]);
        }
        __syncthreads();
        if (t0 + KS_CHUNK < nt) {
          load_chunk(xw, dt, t0 + KS_CHUNK, nt, tid);
          pre_t = t;
          pre_t0 = t0 + KS_CHUNK;
        } else if (t + 1 < t_end) {
          const int ti2 = t_img[t + 1];
          const int nt2 = used_count(kp_count, n_img, max_kp, top, ti2);
          if (nt2 > 0) {
            load_chunk(xw, desc32 + (size_t)ti2 * max_kp * 8, 0, nt2, tid);
            pre_t = t + 1;
            pre_t0 = 0;
          }
        }
        if (!wave_busy) continue;
        const int ntile = min(KS_CHUNK, nt - t0 + 31) >> 5;
        for (int tile = 0; tile < ntile; ++tile) {
          const uint8_t* arow = s_t + (32 * tile + r) * HM_ROWB + 16 * h;
          v16f_t acc[KS_QT];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const v8i_t a = fp4_operand(*reinterpret_cast<const v4i_t*>(arow + 32 * ks));
#pragma unroll
            for (int c = 0; c < KS_QT; ++c)
              acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, fp4_operand(bq[c][ks]), ks == 0 ? zero : acc[c], 4, 4,
                                                                       0, HM_SCALE_A, 0, HM_SCALE_A);
          }
          if (t0 + 32 * tile + 32 > nt) {                 // wave-uniform: rows past the train count are no neighbours
            const int tr = t0 + 32 * tile + 4 * h;        // train index of this lane's row 0
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
              if (tr + (reg & 3) + 8 * (reg >> 2) >= nt) {
#pragma unroll
                for (int c = 0; c < KS_QT; ++c) acc[c][reg] = -INFINITY;
              }
          }
#pragma unroll
          for (int c = 0; c < KS_QT; ++c) cm[c] = tile_max(acc[c], cm[c]);
        }
      }
      if (wave_busy) {                                    // wave-uniform: every lane takes part in the shuffles and ballots
        int hits = 0;
#pragma unroll
        for (int c = 0; c < KS_QT; ++c) {
          const float m = fmaxf(cm[c], __shfl_xor(cm[c], 32));
          hits += __popcll(__ballot(h == 0 && m >= min_dot && q0 + 32 * c < nq));
        }
        if (lane == 0 && hits > 0) atomicAdd(&S[(size_t)q * n_t + t], hits);
      }
    }
  }
}

}  // namespace

extern "C" int vus_keyframe_similarity(const uint64_t* desc, const int* kp_count, int n_img, int max_kp, const int* q_img,
                                       int n_q, const int* t_img, int n_t, const int* t_limit, int top, int max_dist,
                                       int32_t* S, void* stream) {
  VUS_REQUIRE(n_img >= 1, "n_img=%d must be at least 1", n_img);
  VUS_REQUIRE(n_q >= 1, "n_q=%d must be at least 1", n_q);
  VUS_REQUIRE(n_t >= 1, "n_t=%d must be at least 1", n_t);
  VUS_REQUIRE((long long)n_q * n_t <= 2147483647ll, "n_q * n_t = %lld exceeds 2^31 - 1", (long long)n_q * n_t);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= VUS_RETRIEVAL_MAX_KP, "max_kp=%d out of range [1, %d]", max_kp, VUS_RETRIEVAL_MAX_KP);
  VUS_REQUIRE(top >= 1 && top <= max_kp, "top=%d out of range [1, max_kp=%d]", top, max_kp);
  VUS_REQUIRE(max_dist >= 0 && max_dist <= 256, "max_dist=%d out of range [0, 256]", max_dist);
  VUS_REQUIRE(desc != nullptr, "desc is null");
  VUS_REQUIRE(kp_count != nullptr, "kp_count is null");
  VUS_REQUIRE(q_img != nullptr, "q_img is null");
  VUS_REQUIRE(t_img != nullptr, "t_img is null");
  VUS_REQUIRE(S != nullptr, "S is null");
  hipStream_t st = vus::as_stream(stream);
  VUS_CHECK_HIP(hipMemsetAsync(S, 0, sizeof(int32_t) * (size_t)n_q * n_t, st));
  const int n_tb = (n_t + KS_TB - 1) / KS_TB, n_qb = (top + KS_QWG - 1) / KS_QWG;
  const long long n_work = (long long)n_q * n_tb * n_qb;
  keyframe_similarity_kernel<<<(unsigned)std::min(n_work, KS_MAX_GRID), 256, 0, st>>>(
      reinterpret_cast<const uint32_t*>(desc), kp_count, n_img, max_kp, q_img, n_q, t_img, n_t, t_limit, top,
      (float)(256 - 2 * max_dist), n_qb, n_work, S);
  VUS_CHECK_LAUNCH("keyframe_similarity");
  return VUS_OK;
}
