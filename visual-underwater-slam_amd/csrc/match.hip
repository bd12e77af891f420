// match.hip -- brute-force Hamming matching of the stereo ORB front-end (frontend_common.h): row-gated (stereo), ungated
// (tracks, on the matrix cores), and the cross-check.
//
// Design notes (MI355X):
//  * hamming_match keeps the train descriptors in LDS (broadcast reads) and one query per lane.
#include "frontend_common.h"
#include "fp4_hamming.h"
#include <algorithm>

namespace {

// ---------------------------------------------------------------------------------------------
// Brute-force Hamming: one query per lane, train descriptors staged in LDS tiles.
#ifndef VUS_MT
#define VUS_MT 512
#endif
constexpr int MT = VUS_MT;  // train tile

template <bool GATE>
__global__ __launch_bounds__(256) void hamming_match_kernel(
    const uint64_t* __restrict__ desc, const uint32_t* __restrict__ kp_keys,
    const int* __restrict__ kp_count, int max_kp, int W, int Hrows, const int* __restrict__ q_index,
    const int* __restrict__ t_index, int max_dy, int min_disp, int max_disp, int max_dist,
    int32_t* __restrict__ idx_out, int32_t* __restrict__ dist_out) {
  __shared__ uint64_t s_desc[MT * 4];
  __shared__ int s_xy[MT];
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const int qi = q_index[p], ti = t_index[p];
  const int i = blockIdx.x * 256 + tid;
  const int nq = min(kp_count[qi], max_kp), nt = min(kp_count[ti], max_kp);   // a count above max_kp is clamped
  bool active = i < nq;
  uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
  int yq = 0, xq = 0;
  if (active) {
    const uint64_t* dq = desc + ((size_t)qi * max_kp + i) * 4;
    q0 = dq[0]; q1 = dq[1]; q2 = dq[2]; q3 = dq[3];
    if (GATE) {   // without a gate the positions are not read
      uint32_t pq = kp_keys[(size_t)qi * max_kp + i] & VUS_KEY_POS_MASK;
      yq = (int)(pq / (uint32_t)W);
      xq = (int)(pq - (uint32_t)yq * (uint32_t)W);
      active = yq < Hrows;   // a query outside the image takes no part
    }
  }
  int best = 1 << 20, bidx = -1;
  const uint64_t* dt = desc + (size_t)ti * max_kp * 4;
  const uint32_t* kt = kp_keys + (size_t)ti * max_kp;
  for (int t0 = 0; t0 < nt; t0 += MT) {
    const int tn = min(MT, nt - t0);
    __syncthreads();
    for (int k = tid; k < tn * 4; k += 256) s_desc[k] = dt[(size_t)t0 * 4 + k];
    if (GATE) {
      for (int k = tid; k < tn; k += 256) {
        uint32_t pt = kt[t0 + k] & VUS_KEY_POS_MASK;
        int yt = (int)(pt / (uint32_t)W);
        // a train keypoint outside the image fails the gate: -1 is no (y, x) of a row below Hrows <= 65535
        s_xy[k] = yt < Hrows ? (yt << 16) | (int)(pt - (uint32_t)yt * (uint32_t)W) : -1;
      }
    }
    __syncthreads();
    if (active) {
      for (int j = 0; j < tn; ++j) {
        int dist = __popcll(q0 ^ s_desc[4 * j]) + __popcll(q1 ^ s_desc[4 * j + 1]) +
                   __popcll(q2 ^ s_desc[4 * j + 2]) + __popcll(q3 ^ s_desc[4 * j + 3]);
        bool ok = true;
        if (GATE) {
          int xy = s_xy[j];
          int dy = yq - (int)((unsigned)xy >> 16), dx = xq - (xy & 0xFFFF);
          ok = xy != -1 && dy <= max_dy && dy >= -max_dy && dx >= min_disp && dx <= max_disp;
        }
        if (ok && dist < best) { best = dist; bidx = t0 + j; }
      }
    }
  }
  if (i < max_kp) {
    if (bidx < 0) best = 512;
    else if (best > max_dist) bidx = -1;
    idx_out[(size_t)p * max_kp + i] = bidx;
    dist_out[(size_t)p * max_kp + i] = best;
  }
}

// ---------------------------------------------------------------------------------------------
// Row-gated Hamming (stereo): only train keypoints within max_dy rows of the query can match, so the
// train set is bucketed by image row in LDS (counting sort) and each query lane visits the ~30
// keypoints of its 2*max_dy+1 rows instead of all 2000.  Ties are broken on the train index
// explicitly, so the visiting order does not matter and the result equals the brute-force scan.
// This variant keeps only the index table in LDS and gathers the train descriptors from global memory, 256 queries
// per workgroup: it serves the sizes whose train set does not fit into LDS whole (hamming_match_rows_kernel below).
__global__ __launch_bounds__(256) void hamming_match_rows_gather_kernel(
    const uint64_t* __restrict__ desc, const uint32_t* __restrict__ kp_keys,
    const int* __restrict__ kp_count, int max_kp, int W, int Hrows, const int* __restrict__ q_index,
    const int* __restrict__ t_index, int max_dy, int min_disp, int max_disp, int max_dist,
    int32_t* __restrict__ idx_out, int32_t* __restrict__ dist_out) {
  extern __shared__ int s_dyn[];
  int* s_start = s_dyn;                         // [Hrows + 1] first slot of every row
  int* s_cursor = s_dyn + (Hrows + 1);          // [Hrows]
  int* s_list = s_cursor + Hrows;               // [max_kp] train indices grouped by row
  int* s_xy = s_list + max_kp;                  // [max_kp] (y << 16) | x per train index
  __shared__ int s_wsum[4];
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const int qi = q_index[p], ti = t_index[p];
  const int i = blockIdx.x * 256 + tid;
  const int nq = min(kp_count[qi], max_kp), nt = min(kp_count[ti], max_kp);
  const uint32_t* kt = kp_keys + (size_t)ti * max_kp;
  for (int r = tid; r <= Hrows; r += 256) s_start[r] = 0;
  __syncthreads();
  // a train keypoint outside the image (row >= Hrows: VUS_KEY_INVALID is one) is in no bucket; s_xy = -1 tells the
  // placing pass below to skip it as well ((y << 16) | x >= 0: the index table only fits into LDS for Hrows < 12288)
  for (int j = tid; j < nt; j += 256) {
    const uint32_t pt = kt[j] & VUS_KEY_POS_MASK;
    const int yt = (int)(pt / (uint32_t)W);
    const bool inside = yt < Hrows;
    s_xy[j] = inside ? (yt << 16) | (int)(pt - (uint32_t)yt * (uint32_t)W) : -1;
    if (inside) atomicAdd(&s_start[yt + 1], 1);
  }
  __syncthreads();
  // inclusive scan of s_start[1..Hrows] (counts) -> row starts; 256 threads, chunked
  {
    const int per = (Hrows + 255) / 256;
    const int b = 1 + tid * per, e = min(Hrows + 1, b + per);
    int sum = 0;
    for (int r = b; r < e; ++r) sum += s_start[r];
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int v = __shfl_up(incl, o);
      if ((tid & 63) >= o) incl += v;
    }
    if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) base += s_wsum[w];
    for (int r = b; r < e; ++r) { base += s_start[r]; s_start[r] = base; }
  }
  __syncthreads();
  for (int r = tid; r < Hrows; r += 256) s_cursor[r] = s_start[r];
  __syncthreads();
  for (int j = tid; j < nt; j += 256)
    if (s_xy[j] >= 0) s_list[atomicAdd(&s_cursor[s_xy[j] >> 16], 1)] = j;
  __syncthreads();

  int best = 1 << 20, bidx = -1;
  if (i < nq) {
    const uint64_t* dq = desc + ((size_t)qi * max_kp + i) * 4;
    const uint64_t q0 = dq[0], q1 = dq[1], q2 = dq[2], q3 = dq[3];
    const uint32_t pq = kp_keys[(size_t)qi * max_kp + i] & VUS_KEY_POS_MASK;
    const int yq = (int)(pq / (uint32_t)W), xq = (int)(pq - (uint32_t)yq * (uint32_t)W);
    const int r0 = max(0, yq - max_dy), r1 = min(Hrows - 1, yq + max_dy);
    const uint64_t* dt = desc + (size_t)ti * max_kp * 4;
    if (yq < Hrows && r0 <= r1) {   // a query outside the image visits nothing
      for (int c = s_start[r0]; c < s_start[r1 + 1]; ++c) {
        const int j = s_list[c];
        const int dx = xq - (s_xy[j] & 0xFFFF);
        if (dx < min_disp || dx > max_disp) continue;
        const uint64_t* d = dt + (size_t)j * 4;
        const int dist = __popcll(q0 ^ d[0]) + __popcll(q1 ^ d[1]) + __popcll(q2 ^ d[2]) + __popcll(q3 ^ d[3]);
        if (dist < best || (dist == best && j < bidx)) { best = dist; bidx = j; }
      }
    }
  }
  if (i < max_kp) {
    if (bidx < 0) best = 512;
    else if (best > max_dist) bidx = -1;
    idx_out[(size_t)p * max_kp + i] = bidx;
    dist_out[(size_t)p * max_kp + i] = best;
  }
}

// ---------------------------------------------------------------------------------------------
// Row-gated Hamming with the whole train set in LDS: ONE workgroup per pair buckets the train keypoints by row once
// and stores them in row order -- descriptor (32 B), x and original index -- so a query lane walks one contiguous LDS
// range, start[y - max_dy] .. start[y + max_dy + 1], tests the disparity on the LDS-resident x and only then reads the
// descriptor, also from LDS.  At 2000 keypoints and 720 rows that is 78 KB: two workgroups per CU.
// A thread stages at most HR_PER train keypoints (blockDim.x * HR_PER >= max_kp, the host's choice).
constexpr int HR_THREADS = 1024;
constexpr int HR_PER = 2;

__host__ __device__ constexpr size_t hamming_rows_lds(int max_kp, int h_rows) {
  return (size_t)max_kp * 32 + (size_t)max_kp * 4 + ((size_t)2 * h_rows + 1) * 4;
}

__global__ __launch_bounds__(HR_THREADS) void hamming_match_rows_kernel(
    const uint64_t* __restrict__ desc, const uint32_t* __restrict__ kp_keys,
    const int* __restrict__ kp_count, int max_kp, int W, int Hrows, const int* __restrict__ q_index,
    const int* __restrict__ t_index, int max_dy, int min_disp, int max_disp, int max_dist,
    int32_t* __restrict__ idx_out, int32_t* __restrict__ dist_out) {
  extern __shared__ uint4 s_rows[];
  uint4* s_desc = s_rows;                                               // [max_kp][2] descriptors in row order
  uint32_t* s_xi = reinterpret_cast<uint32_t*>(s_desc + 2 * (size_t)max_kp);   // [max_kp] x | train index << 16
  int* s_start = reinterpret_cast<int*>(s_xi + max_kp);                 // [Hrows + 1] first slot of every row
  int* s_cursor = s_start + (Hrows + 1);                                // [Hrows]
  __shared__ int s_wsum[HR_THREADS / 64];
  const int tid = threadIdx.x, T = blockDim.x;
  const int p = blockIdx.x;
  const int qi = q_index[p], ti = t_index[p];
  const int nq = min(kp_count[qi], max_kp), nt = min(kp_count[ti], max_kp);
  const uint32_t* kt = kp_keys + (size_t)ti * max_kp;
  const uint64_t* dt = desc + (size_t)ti * max_kp * 4;
  for (int r = tid; r <= Hrows; r += T) s_start[r] = 0;
  __syncthreads();
  // this thread's train keypoints: row count, and the descriptor on its way while the rows are scanned
  // t_yx stays -1 for a slot past the count and for a train keypoint outside the image (row >= Hrows: VUS_KEY_INVALID
  // is one), which is in no bucket: the placing pass below skips exactly these ((y << 16) | x >= 0: the train set only
  // fits into LDS for Hrows < 12288)
  int t_yx[HR_PER];
  uint64_t t_d[HR_PER][4];
#pragma unroll
  for (int u = 0; u < HR_PER; ++u) {
    const int j = tid + u * T;
    t_yx[u] = -1;
    if (j < nt) {
      const uint32_t pt = kt[j] & VUS_KEY_POS_MASK;
      const uint32_t yt = pt / (uint32_t)W;
      if (yt < (uint32_t)Hrows) {
        t_yx[u] = (int)(yt << 16) | (int)(pt - yt * (uint32_t)W);
#pragma unroll
        for (int w = 0; w < 4; ++w) t_d[u][w] = dt[(size_t)j * 4 + w];
        atomicAdd(&s_start[yt + 1], 1);
      }
    }
  }
  __syncthreads();
  // inclusive scan of s_start[1 .. Hrows] (counts) -> row starts, chunked over the threads; the cursors start there
  {
    const int per = (Hrows + T - 1) / T;
    const int b = min(Hrows + 1, 1 + tid * per), e = min(Hrows + 1, b + per);
    int sum = 0;
    for (int r = b; r < e; ++r) sum += s_start[r];
    const int incl = wave_incl_scan(sum);
    if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) base += s_wsum[w];
    for (int r = b; r < e; ++r) {
      base += s_start[r];
      s_start[r] = base;
      if (r < Hrows) s_cursor[r] = base;
    }
    if (tid == 0) s_cursor[0] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < HR_PER; ++u) {
    const int j = tid + u * T;
    if (t_yx[u] >= 0) {
      const int c = atomicAdd(&s_cursor[t_yx[u] >> 16], 1);
      s_xi[c] = (uint32_t)(t_yx[u] & 0xFFFF) | ((uint32_t)j << 16);
      s_desc[2 * c] = make_uint4((uint32_t)t_d[u][0], (uint32_t)(t_d[u][0] >> 32), (uint32_t)t_d[u][1], (uint32_t)(t_d[u][1] >> 32));
      s_desc[2 * c + 1] = make_uint4((uint32_t)t_d[u][2], (uint32_t)(t_d[u][2] >> 32), (uint32_t)t_d[u][3], (uint32_t)(t_d[u][3] >> 32));
    }
  }
  __syncthreads();

  for (int i = tid; i < max_kp; i += T) {
    int best = 1 << 20, bidx = -1;
    if (i < nq) {
      const uint64_t* dq = desc + ((size_t)qi * max_kp + i) * 4;
      const uint64_t q0 = dq[0], q1 = dq[1], q2 = dq[2], q3 = dq[3];
      const uint32_t pq = kp_keys[(size_t)qi * max_kp + i] & VUS_KEY_POS_MASK;
      const int yq = (int)(pq / (uint32_t)W), xq = (int)(pq - (uint32_t)yq * (uint32_t)W);
      const int r0 = max(0, yq - max_dy), r1 = min(Hrows - 1, yq + max_dy);
      if (yq < Hrows && r0 <= r1) {   // a query outside the image visits nothing
        const int c_end = s_start[r1 + 1];
        for (int c = s_start[r0]; c < c_end; ++c) {
          const uint32_t xi = s_xi[c];
          const int dx = xq - (int)(xi & 0xFFFFu);
          if (dx < min_disp || dx > max_disp) continue;
          const uint4 d0 = s_desc[2 * c], d1 = s_desc[2 * c + 1];
          const int dist = __popcll(q0 ^ (d0.x | ((uint64_t)d0.y << 32))) + __popcll(q1 ^ (d0.z | ((uint64_t)d0.w << 32))) +
                           __popcll(q2 ^ (d1.x | ((uint64_t)d1.y << 32))) + __popcll(q3 ^ (d1.z | ((uint64_t)d1.w << 32)));
          const int j = (int)(xi >> 16);
          if (dist < best || (dist == best && j < bidx)) { best = dist; bidx = j; }
        }
      }
    }
    if (bidx < 0) best = 512;
    else if (best > max_dist) bidx = -1;
    idx_out[(size_t)p * max_kp + i] = bidx;
    dist_out[(size_t)p * max_kp + i] = best;
  }
}

// ---------------------------------------------------------------------------------------------
// Ungated brute-force matcher on the matrix cores.  With the descriptor bits as +-1 values,
// dot(q, t) = 256 - 2 * Hamming(q, t) exactly, so argmin Hamming = argmax dot: the 2000 x 2000 x 256-bit
// all-pairs problem of one image pair is a GEMM (the VALU version is bound by the v_bcnt issue rate).
// +-1 is exact in FP4 (E2M1: +1.0 = 0x2, -1.0 = 0xA), so the product runs on the block-scaled FP4 MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4: the cycles of the int8 32x32x32 form at twice the K, four MFMAs per
// 32x32 tile over K = 256.  Rows of a tile = train descriptors (A operand, expanded into LDS once per
// HM_CHUNK-train chunk and shared by the four waves; the next chunk's words are loaded while the current one's
// tiles run), columns = the wave's 32 * HM_QT queries (B operand, expanded once into registers).  A and B use the same lane -> k map, so only the C layout
// (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) matters.
//
// Keys.  Every accumulator is an integer of magnitude < 2^24, exact in f32 in any summation order: the
// B block scale 2^HM_KEY_SHIFT (= HM_CHUNK) puts the factor HM_CHUNK on the dot product, and the C input of
// a tile's first MFMA is HM_CHUNK - 1 - row, so a value is HM_CHUNK * dot + (HM_CHUNK - 1 - row).  Within
// a chunk the running best is kept in f32 as (best chunk key + 32 * tile), chunk key = HM_CHUNK * dot +
// (HM_CHUNK - 1 - local train index): one max3 tree per tile and column tile, seeded with the previous
// best + 32.  Once per chunk it becomes the global key (dot << 16) | (0xFFFF - train index), running
// signed max = smallest distance, ties to the lowest train index -- the brute-force result, bit for bit.
// The vector types, the row pitch HM_ROWB, the unit scale word HM_SCALE_A and the expansion helpers (spread_fp4, spread_word,
// fp4_operand) are shared with the keyframe retrieval (retrieve.hip): fp4_hamming.h.
#ifndef VUS_HM_CHUNK
#define VUS_HM_CHUNK 128
#endif
constexpr int HM_CHUNK = VUS_HM_CHUNK;   // trains expanded per LDS chunk
constexpr int HM_KEY_SHIFT = HM_CHUNK == 256 ? 8 : HM_CHUNK == 128 ? 7 : HM_CHUNK == 64 ? 6 : -1;
static_assert(HM_KEY_SHIFT > 0, "HM_CHUNK must be 64, 128 or 256");
// E8M0 block scales, every byte the same: HM_SCALE_A = 2^0 (trains) and 2^HM_KEY_SHIFT (queries)
constexpr int HM_SCALE_B = (int)(0x01010101u * (0x7F + HM_KEY_SHIFT));

#ifndef VUS_HM_QT
#define VUS_HM_QT 4
#endif
constexpr int HM_QT = VUS_HM_QT;         // 32-query column tiles per wave (A fragments and the chunk expansion are shared)
constexpr int HM_QWG = 4 * 32 * HM_QT;   // queries per workgroup

__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// running chunk best of one column tile after one more tile: max over the 16 keys of this lane's rows and prev + 32
__device__ __forceinline__ float tile_best(const v16f_t& acc, float prev) {
  const float m0 = max3f(acc[0], acc[1], acc[2]), m1 = max3f(acc[3], acc[4], acc[5]), m2 = max3f(acc[6], acc[7], acc[8]),
              m3 = max3f(acc[9], acc[10], acc[11]), m4 = max3f(acc[12], acc[13], acc[14]),
              m5 = max3f(acc[15], prev + 32.0f, m0);
  return max3f(max3f(m1, m2, m3), m4, m5);
}

// waves_per_eu(3): 166 registers, no spill, 3 waves per SIMD (172 and 2 waves without the hint: 0.38 vs 0.36 ms)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void hamming_match_mfma_kernel(
    const uint32_t* __restrict__ desc32, const int* __restrict__ kp_count, int max_kp, const int* __restrict__ q_index,
    const int* __restrict__ t_index, int max_dist, int32_t* __restrict__ idx_out, int32_t* __restrict__ dist_out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_t[HM_CHUNK * HM_ROWB];
  __shared__ uint32_t s_lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_lut[tid] = spread_fp4(tid);
  __syncthreads();
  const int r = lane & 31, h = lane >> 5;
  const int p = blockIdx.y;
  const int qi = q_index[p], ti = t_index[p];
  const int nq = min(max(kp_count[qi], 0), max_kp);          // counts are clamped to [0, max_kp] as on every other path
  const int wq0 = blockIdx.x * HM_QWG + 32 * HM_QT * wave;   // first query of this wave
  const int q0 = wq0 + r;                                     // column tile c holds query q0 + 32 c
  // a workgroup without queries skips the trains; a wave without queries only helps expand them
  const int nt = blockIdx.x * HM_QWG < nq ? min(max(kp_count[ti], 0), max_kp) : 0;
  const bool wave_busy = wq0 < nq;
  // B fragments: MFMA ks, lane half h <-> descriptor word 2 ks + h
  v4i_t bq[HM_QT][4];
#pragma unroll
  for (int c = 0; c < HM_QT; ++c) {
    const int q = q0 + 32 * c;
    const uint32_t* dq = desc32 + ((size_t)qi * max_kp + min(q, max_kp - 1)) * 8 + h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bq[c][ks] = spread_word(s_lut, dq[2 * ks]);   // a column past nq is never written
  }
  // initial value of a tile's accumulators: HM_CHUNK - 1 - (row of the value inside this lane's sixteen)
  v16f_t cinit;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) cinit[reg] = (float)(HM_CHUNK - 1 - ((reg & 3) + 8 * (reg >> 2)));
  int best[HM_QT];
#pragma unroll
  for (int c = 0; c < HM_QT; ++c) best[c] = INT_MIN;
  // the chunk's (train, 32-bit word) items of this thread, loaded one chunk ahead; a row past nt loads row nt - 1, whose
  // keys the epilogue masks
  const uint32_t* dt = desc32 + (size_t)ti * max_kp * 8;
  constexpr int HM_ITEMS = HM_CHUNK * 8 / 256;
  uint32_t xw[HM_ITEMS];
#pragma unroll
  for (int u = 0; u < HM_ITEMS; ++u) xw[u] = nt > 0 ? dt[(size_t)min((tid + 256 * u) >> 3, nt - 1) * 8 + (tid & 7)] : 0u;
  for (int t0 = 0; t0 < nt; t0 += HM_CHUNK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HM_ITEMS; ++u) {
      const int item = tid + 256 * u;
      *reinterpret_cast<v4i_t*>(s_t + (item >> 3) * HM_ROWB + 16 * (item & 7)) = spread_word(s_lut, xw[u]);
    }
    __syncthreads();
    if (t0 + HM_CHUNK < nt) {
#pragma unroll
      for (int u = 0; u < HM_ITEMS; ++u)
        xw[u] = dt[(size_t)min(t0 + HM_CHUNK + ((tid + 256 * u) >> 3), nt - 1) * 8 + (tid & 7)];
    }
    if (!wave_busy) continue;
    const int ntile = min(HM_CHUNK, nt - t0 + 31) >> 5;
    float cb[HM_QT];                                     // chunk best + 32 * tile
#pragma unroll
    for (int c = 0; c < HM_QT; ++c) cb[c] = -INFINITY;
    for (int tile = 0; tile < ntile; ++tile) {
      const uint8_t* arow = s_t + (32 * tile + r) * HM_ROWB + 16 * h;
      v16f_t acc[HM_QT];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const v8i_t a = fp4_operand(*reinterpret_cast<const v4i_t*>(arow + 32 * ks));
#pragma unroll
        for (int c = 0; c < HM_QT; ++c)
          acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, fp4_operand(bq[c][ks]), ks == 0 ? cinit : acc[c],
                                                                   4, 4, 0, HM_SCALE_A, 0, HM_SCALE_B);
      }
      if (t0 + 32 * tile + 32 > nt) {                   // wave-uniform: rows past the train count cannot win
        const int tb = t0 + 32 * tile + 4 * h;          // train index of this lane's row 0
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          if (tb + (reg & 3) + 8 * (reg >> 2) >= nt) {
#pragma unroll
            for (int c = 0; c < HM_QT; ++c) acc[c][reg] = -INFINITY;
          }
      }
#pragma unroll
      for (int c = 0; c < HM_QT; ++c) cb[c] = tile_best(acc[c], cb[c]);
    }
    // chunk key -> global key (a lane half whose rows of the chunk all lie past nt keeps -inf)
#pragma unroll
    for (int c = 0; c < HM_QT; ++c) {
      if (!(cb[c] > -INFINITY)) continue;
      const int k = (int)(cb[c] - 32.0f * (ntile - 1));
      const int train = t0 + 4 * h + (HM_CHUNK - 1 - (k & (HM_CHUNK - 1)));
      best[c] = max(best[c], (k >> HM_KEY_SHIFT) * 65536 + (0xFFFF - train));
    }
  }
#pragma unroll
  for (int c = 0; c < HM_QT; ++c) {
    const int b2 = max(best[c], __shfl_xor(best[c], 32));
    const int q = q0 + 32 * c;
    if (h == 0 && q < max_kp) {
      int bidx = -1, bd = 512;
      const int dot = b2 >> 16;
      if (q < nq && nt > 0 && dot >= -256) {
        bd = (256 - dot) >> 1;
        bidx = 0xFFFF - (b2 & 0xFFFF);
        if (bd > max_dist) bidx = -1;
      }
      idx_out[(size_t)p * max_kp + q] = bidx;
      dist_out[(size_t)p * max_kp + q] = bd;
    }
  }
}

}  // namespace

extern "C" int vus_hamming_match(const uint64_t* desc, const uint32_t* kp_keys, const int* kp_count,
                                 int max_kp, int H, int W, const int* q_index, const int* t_index, int n_pairs,
                                 int max_dy, int min_disp, int max_disp, int max_dist,
                                 int32_t* idx_out, int32_t* dist_out, void* stream) {
  VUS_REQUIRE(desc && kp_keys && kp_count && q_index && t_index && idx_out && dist_out, "null buffer");
  VUS_REQUIRE(max_kp >= 1 && W >= 1 && W < 65536 && H >= 1 && H < 65536, "max_kp=%d H=%d W=%d", max_kp, H, W);
  VUS_REQUIRE(n_pairs >= 0 && n_pairs <= 65535, "n_pairs=%d out of range [0, 65535]", n_pairs);
  if (n_pairs == 0) return VUS_OK;
  // two keypoints inside the image lie fewer than H <= 65535 rows apart, so a wider gate admits the same pairs; the
  // rows kernels compute yq + max_dy in int
  max_dy = std::min(max_dy, 65535);
  dim3 grid((max_kp + 255) / 256, n_pairs);
  const int h_rows = H;   // the gated kernels bucket the train keypoints by image row
  const size_t lds_all = hamming_rows_lds(max_kp, h_rows);                                     // train set resident in LDS
  const size_t lds = sizeof(int) * ((size_t)2 * h_rows + 1 + 2 * (size_t)max_kp);             // index table only
  if (max_dy >= 0 && max_kp <= HR_THREADS * HR_PER && lds_all <= 96 * 1024) {
    const int threads = std::min(HR_THREADS, (max_kp + 63) / 64 * 64);
    if (lds_all > 48 * 1024)
      VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hamming_match_rows_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_all));
    hamming_match_rows_kernel<<<n_pairs, threads, lds_all, vus::as_stream(stream)>>>(
        desc, kp_keys, kp_count, max_kp, W, h_rows, q_index, t_index, max_dy, min_disp, max_disp, max_dist, idx_out,
        dist_out);
  } else if (max_dy >= 0 && lds <= 96 * 1024) {
    if (lds > 48 * 1024)
      VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hamming_match_rows_gather_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hamming_match_rows_gather_kernel<<<grid, 256, lds, vus::as_stream(stream)>>>(
        desc, kp_keys, kp_count, max_kp, W, h_rows, q_index, t_index, max_dy, min_disp, max_disp, max_dist, idx_out,
        dist_out);
  } else {
    if (max_dy >= 0)
      hamming_match_kernel<true><<<grid, 256, 0, vus::as_stream(stream)>>>(
          desc, kp_keys, kp_count, max_kp, W, h_rows, q_index, t_index, max_dy, min_disp, max_disp, max_dist, idx_out, dist_out);
    else if (max_kp <= 65535)   // ungated: FP4 GEMM formulation on the matrix cores
      hamming_match_mfma_kernel<<<dim3((max_kp + HM_QWG - 1) / HM_QWG, n_pairs), 256, 0, vus::as_stream(stream)>>>(
          reinterpret_cast<const uint32_t*>(desc), kp_count, max_kp, q_index, t_index, max_dist, idx_out, dist_out);
    else
      hamming_match_kernel<false><<<grid, 256, 0, vus::as_stream(stream)>>>(
          desc, kp_keys, kp_count, max_kp, W, h_rows, q_index, t_index, max_dy, min_disp, max_disp, max_dist, idx_out, dist_out);
  }
  VUS_CHECK_LAUNCH("hamming_match");
  return VUS_OK;
}

namespace {

__global__ void cross_check_kernel(const int32_t* __restrict__ idx_fwd, const int32_t* __restrict__ idx_bwd, int max_kp,
                                   long long total, int32_t* __restrict__ idx_out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long long row = t / max_kp;
  const int i = (int)(t - row * max_kp);
  const int32_t j = idx_fwd[t];
  idx_out[t] = (j >= 0 && j < max_kp && idx_bwd[row * max_kp + j] == i) ? j : -1;
}

}  // namespace

extern "C" int vus_cross_check(const int32_t* idx_fwd, const int32_t* idx_bwd, int n_pairs, int max_kp,
                               int32_t* idx_out, void* stream) {
  VUS_REQUIRE(idx_fwd && idx_bwd && idx_out, "null buffer");
  VUS_REQUIRE(n_pairs >= 0 && max_kp >= 1, "n_pairs=%d max_kp=%d", n_pairs, max_kp);
  const long long total = (long long)n_pairs * max_kp;
  if (total == 0) return VUS_OK;
  cross_check_kernel<<<(unsigned)((total + 255) / 256), 256, 0, vus::as_stream(stream)>>>(idx_fwd, idx_bwd, max_kp, total,
                                                                                       idx_out);
  VUS_CHECK_LAUNCH("cross_check");
  return VUS_OK;
}
