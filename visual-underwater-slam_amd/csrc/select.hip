// select.hip -- keypoint selection of the stereo ORB front-end (frontend_common.h): exact top-K, and the grid-bucketed form.
//
// Design notes (MI355X):
//  * select_topk is an exact MSB radix select (score byte, then the boundary bucket alone) + a bitonic sort held in
//    registers, one workgroup per image.
#include "frontend_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Exact top-K: the max_kp smallest keys of one image, ascending.  One workgroup of sort_n / 8 threads per image
// (sort_n = max_kp rounded up to a power of two, 2048 at least: 256 to 1024 threads).
//  * The score byte (bits 24 .. 31) decides nearly everything: one histogram pass over it (a histogram per wave, summed
//    and scanned by wave 0) finds the bucket b that holds the max_kp-th smallest key.  Keys of lower buckets are kept
//    outright; only the keys of bucket b -- typically tens -- are looked at again.
//  * Up to SEL_RANK_MAX boundary keys are ranked against each other in LDS.  A longer boundary bucket (an image with
//    one score) takes three more 8-bit radix passes over the list in global memory, as every image did before.
//  * The candidates are read from global memory once: a lane keeps its first SEL_CACHE in registers.  The tail of a
//    longer list (more than SEL_CACHE * blockDim.x candidates) is streamed again in the second pass.
//  * The kept keys (all below the threshold key T, so fewer than max_kp) are sorted by a bitonic network with SEL_E keys
//    per lane in registers: partner distances below SEL_E are exchanges inside a lane, those below 64 * SEL_E are wave
//    shuffles, and only the remaining ones (3 of the 66 stages at 2048 keys) go through LDS between two barriers.
//    The output is those keys, then T as often as the list holds it up to max_kp (keys are unique except for
//    VUS_KEY_INVALID entries of an overflowed list), then VUS_KEY_INVALID.
constexpr int SEL_THREADS = 1024;   // select_grid_kernel; the largest workgroup of select_topk_kernel
constexpr int SEL_E = 8;            // keys per lane in the register sort
constexpr int SEL_CACHE = 16;       // candidates per lane kept in registers between the two passes
constexpr int SEL_RANK_MAX = 256;   // boundary-bucket keys ranked directly in LDS

// Wave 0: sum the n_copies histograms of 256 bins, find the bin that holds the kk-th smallest key (kk >= 1, at most the
// number of keys counted) and publish it: *s_thr |= bin << shift, *s_k = rank inside the bin, *s_nb = keys in the bin.
__device__ __forceinline__ void sel_pick_bucket(const int* s_hist, int n_copies, int kk, int shift, uint32_t* s_thr, int* s_k,
                                                int* s_nb) {
  const int lane = threadIdx.x;   // callers pass threads 0 .. 63 only
  int h[4], tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int v = 0;
    for (int w = 0; w < n_copies; ++w) v += s_hist[w * 256 + 4 * lane + q];
    h[q] = v;
    tot += v;
  }
  int excl = wave_incl_scan(tot) - tot;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (excl < kk && kk <= excl + h[q]) {   // exactly one (lane, q)
      *s_thr |= (uint32_t)(4 * lane + q) << shift;
      *s_k = kk - excl;
      *s_nb = h[q];
    }
    excl += h[q];
  }
}

// Append k to s_sort for the lanes with `take` set: one LDS atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void sel_append(bool take, uint32_t k, uint32_t* s_sort, int sort_n, int* s_out) {
  const uint64_t m = __ballot(take);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(s_out, __popcll(m));
  base = __shfl(base, leader);
  const int p = base + __popcll(m & ((1ull << lane) - 1));
  if (take && p < sort_n) s_sort[p] = k;
}

__global__ __launch_bounds__(SEL_THREADS) void select_topk_kernel(
    const uint32_t* __restrict__ cand_keys, const int* __restrict__ cand_count, int cand_cap,
    int max_kp, int sort_n, uint32_t* __restrict__ kp_keys, int* __restrict__ kp_count) {
  extern __shared__ uint32_t s_sort[];              // [sort_n] kept keys, then the exchange buffer of the sort
  __shared__ uint32_t s_bnd[SEL_RANK_MAX];          // keys of the boundary bucket
  __shared__ uint32_t s_thr;
  __shared__ int s_k, s_nb, s_out, s_fill;
  const int tid = threadIdx.x, NT = blockDim.x, n_waves = NT >> 6;   // the workgroup size NT == sort_n / SEL_E, a multiple of 64
  int* s_hist = reinterpret_cast<int*>(s_sort + sort_n);            // [n_waves][256]
  const int n = blockIdx.x;
  const uint32_t* keys = cand_keys + (size_t)n * cand_cap;
  const int cnt = min(cand_count[n], cand_cap);
  const int K = min(cnt, max_kp);

  uint32_t r[SEL_CACHE];
#pragma unroll
  for (int u = 0; u < SEL_CACHE; ++u) r[u] = tid + u * NT < cnt ? keys[tid + u * NT] : VUS_KEY_INVALID;
  for (int i = tid; i < sort_n; i += NT) s_sort[i] = VUS_KEY_INVALID;

  uint32_t thr = VUS_KEY_INVALID;   // the K-th smallest key
  int n_below = K;                  // how many keys of the output lie below thr
  if (cnt <= max_kp) {              // keep everything: cnt <= max_kp <= sort_n
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SEL_CACHE; ++u)
      if (tid + u * NT < cnt) s_sort[tid + u * NT] = r[u];
    for (int i = tid + SEL_CACHE * NT; i < cnt; i += NT) s_sort[i] = keys[i];
  } else {
    for (int i = tid; i < n_waves * 256; i += NT) s_hist[i] = 0;
    if (tid == 0) { s_thr = 0; s_out = 0; s_fill = 0; }
    __syncthreads();
    int* my_hist = s_hist + (tid >> 6) * 256;
#pragma unroll
    for (int u = 0; u < SEL_CACHE; ++u)
      if (tid + u * NT < cnt) atomicAdd(&my_hist[r[u] >> 24], 1);
    for (int i = tid + SEL_CACHE * NT; i < cnt; i += NT) atomicAdd(&my_hist[keys[i] >> 24], 1);
    __syncthreads();
    if (tid < 64) sel_pick_bucket(s_hist, n_waves, max_kp, 24, &s_thr, &s_k, &s_nb);
    __syncthreads();
    const uint32_t bucket = s_thr >> 24;
    const int kk = s_k, n_bnd = s_nb;
    const bool ranked = n_bnd <= SEL_RANK_MAX;
    // second pass: lower buckets are kept, the boundary bucket is set aside
#pragma unroll
    for (int u = 0; u < SEL_CACHE; ++u) {
      const bool valid = tid + u * NT < cnt;
      const uint32_t b = r[u] >> 24;
      sel_append(valid && b < bucket, r[u], s_sort, sort_n, &s_out);
      if (ranked && valid && b == bucket) s_bnd[atomicAdd(&s_fill, 1) & (SEL_RANK_MAX - 1)] = r[u];   // n_bnd of them
    }
    for (int i0 = SEL_CACHE * NT; i0 < cnt; i0 += NT) {
      const bool valid = i0 + tid < cnt;
      const uint32_t k = valid ? keys[i0 + tid] : VUS_KEY_INVALID;
      sel_append(valid && (k >> 24) < bucket, k, s_sort, sort_n, &s_out);
      if (ranked && valid && (k >> 24) == bucket) s_bnd[atomicAdd(&s_fill, 1) & (SEL_RANK_MAX - 1)] = k;
    }
    __syncthreads();
    if (ranked) {
      // x is the kk-th smallest of the bucket iff  #(y < x) < kk <= #(y <= x);  x lies below it iff #(y <= x) < kk
      for (int t = tid; t < n_bnd; t += NT) {
        const uint32_t x = s_bnd[t];
        int less = 0, leq = 0;
        for (int q = 0; q < n_bnd; ++q) {
          const uint32_t y = s_bnd[q];
          less += y < x;
          leq += y <= x;
        }
        if (less < kk && kk <= leq) { s_thr = x; s_k = kk - less; }   // equal keys write equal values
        if (leq < kk) {
          const int p = atomicAdd(&s_out, 1);
          if (p < sort_n) s_sort[p] = x;
        }
      }
    } else {
      // three more radix passes over the keys that carry the prefix found so far
      uint32_t mask = 0xFF000000u;
      for (int shift = 16; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_thr;
        const int kq = s_k;
        for (int i = tid; i < cnt; i += NT) {
          const uint32_t k = keys[i];
          if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) sel_pick_bucket(s_hist, 1, kq, shift, &s_thr, &s_k, &s_nb);
        mask |= 0xFFu << shift;
        __syncthreads();
      }
      const uint32_t t_key = s_thr;
      for (int i0 = 0; i0 < cnt; i0 += NT) {
        const bool valid = i0 + tid < cnt;
        const uint32_t k = valid ? keys[i0 + tid] : VUS_KEY_INVALID;
        sel_append(valid && (k >> 24) == bucket && k < t_key, k, s_sort, sort_n, &s_out);
      }
    }
    __syncthreads();
    thr = s_thr;
    n_below = max_kp - s_k;   // == s_out
  }
  __syncthreads();

  // bitonic sort, ascending; lane tid holds elements tid * SEL_E .. tid * SEL_E + SEL_E - 1
  uint32_t a[SEL_E];
#pragma unroll
  for (int e = 0; e < SEL_E; ++e) a[e] = s_sort[tid * SEL_E + e];
#pragma unroll
  for (int k = 2; k < SEL_E; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int e = 0; e < SEL_E; ++e) {
        if ((e ^ j) > e) {
          const uint32_t lo = min(a[e], a[e ^ j]), hi = max(a[e], a[e ^ j]);
          const bool up = (e & k) == 0;
          a[e] = up ? lo : hi;
          a[e ^ j] = up ? hi : lo;
        }
      }
    }
  }
  for (int k = SEL_E; k <= sort_n; k <<= 1) {
    const bool up = ((tid * SEL_E) & k) == 0;   // k >= SEL_E: one direction for all of a lane's keys
    for (int j = k >> 1; j >= SEL_E; j >>= 1) {
      const int pj = j / SEL_E;                 // the partner is lane tid ^ pj
      const bool keep_min = ((tid & pj) == 0) == up;
      uint32_t b[SEL_E];
      if (pj >= 64) {                           // another wave: through LDS, [e][tid] so that lanes hit distinct banks
        __syncthreads();
#pragma unroll
        for (int e = 0; e < SEL_E; ++e) s_sort[e * NT + tid] = a[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < SEL_E; ++e) b[e] = s_sort[e * NT + (tid ^ pj)];
      } else {
#pragma unroll
        for (int e = 0; e < SEL_E; ++e) b[e] = (uint32_t)__shfl_xor((int)a[e], pj);
      }
#pragma unroll
      for (int e = 0; e < SEL_E; ++e) a[e] = keep_min ? min(a[e], b[e]) : max(a[e], b[e]);
    }
#pragma unroll
    for (int j = SEL_E >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int e = 0; e < SEL_E; ++e) {
        if ((e ^ j) > e) {
          const uint32_t lo = min(a[e], a[e ^ j]), hi = max(a[e], a[e ^ j]);
          a[e] = up ? lo : hi;
          a[e ^ j] = up ? hi : lo;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < SEL_E; ++e) {
    const int i = tid * SEL_E + e;
    if (i < max_kp) kp_keys[(size_t)n * max_kp + i] = i < n_below ? a[e] : (i < K ? thr : VUS_KEY_INVALID);
  }
  if (tid == 0) kp_count[n] = K;
}

}  // namespace

extern "C" int vus_select_topk(const uint32_t* cand_keys, const int* cand_count, int n_img, int cand_cap,
                               int max_kp, uint32_t* kp_keys, int* kp_count, void* stream) {
  VUS_REQUIRE(cand_keys && cand_count && kp_keys && kp_count, "null buffer");
  VUS_REQUIRE(n_img >= 0, "n_img=%d", n_img);
  VUS_REQUIRE(cand_cap >= 1, "cand_cap=%d", cand_cap);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= 8192, "max_kp=%d out of range [1, 8192]", max_kp);
  if (n_img == 0) return VUS_OK;
  // at least four waves: a small max_kp (a pyramid level's quota) still meets lists of thousands of candidates, which
  // one wave would stream and count alone; max_kp <= 8192 == SEL_THREADS * SEL_E
  int sort_n = 256 * SEL_E;
  while (sort_n < max_kp) sort_n <<= 1;
  const int threads = sort_n / SEL_E;
  const size_t lds = sort_n * sizeof(uint32_t) + (size_t)(threads / 64) * 256 * sizeof(int);   // keys + a histogram per wave
  if (lds > 48 * 1024)   // max_kp 8192: 48 KiB dynamic + 1 KiB static
    VUS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(select_topk_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  select_topk_kernel<<<n_img, threads, lds, vus::as_stream(stream)>>>(
      cand_keys, cand_count, cand_cap, max_kp, sort_n, kp_keys, kp_count);
  VUS_CHECK_LAUNCH("select_topk");
  return VUS_OK;
}

namespace {

// Grid-bucketed selection: one workgroup per image walks the cells in row-major order; per cell, per_cell
// rounds of "smallest key of the cell above the previous pick" (block-wide min), appended in order.
__global__ __launch_bounds__(SEL_THREADS) void select_grid_kernel(const uint32_t* __restrict__ cand_keys,
                                                                  const int* __restrict__ cand_count, int cand_cap,
                                                                  int H, int W, int grid_row, int grid_col, int per_cell,
                                                                  int max_kp, uint32_t* __restrict__ kp_keys,
                                                                  int* __restrict__ kp_count) {
  __shared__ uint32_t s_min[SEL_THREADS / 64];
  __shared__ uint32_t s_pick;
  const int tid = threadIdx.x, n = blockIdx.x;
  const uint32_t* keys = cand_keys + (size_t)n * cand_cap;
  const int cnt = min(cand_count[n], cand_cap);
  uint32_t* o = kp_keys + (size_t)n * max_kp;
  int out = 0;
  for (int cell = 0; cell < grid_row * grid_col && out < max_kp; ++cell) {
    const int cy = cell / grid_col, cx = cell - cy * grid_col;
    uint32_t last = 0;
    bool have_last = false;
    for (int j = 0; j < per_cell && out < max_kp; ++j) {
      uint32_t best = VUS_KEY_INVALID;
      for (int i = tid; i < cnt; i += SEL_THREADS) {
        const uint32_t k = keys[i];
        const int pos = (int)(k & VUS_KEY_POS_MASK), y = pos / W, x = pos - y * W;
        // pos < H * W: a key that names no pixel belongs to no cell (and y * grid_row stays below 2^23)
        if (pos < H * W && y * grid_row / H == cy && x * grid_col / W == cx && !(have_last && k <= last)) best = min(best, k);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));
      if ((tid & 63) == 0) s_min[tid >> 6] = best;
      __syncthreads();
      if (tid == 0) {
        uint32_t b = s_min[0];
        for (int w = 1; w < SEL_THREADS / 64; ++w) b = min(b, s_min[w]);
        s_pick = b;
      }
      __syncthreads();
      const uint32_t pick = s_pick;
      __syncthreads();   // s_pick / s_min are rewritten in the next round
      if (pick == VUS_KEY_INVALID) break;
      if (tid == 0) o[out] = pick;
      ++out;
      last = pick;
      have_last = true;
    }
  }
  for (int i = out + tid; i < max_kp; i += SEL_THREADS) o[i] = VUS_KEY_INVALID;
  if (tid == 0) kp_count[n] = out;
}

}  // namespace

extern "C" int vus_select_grid(const uint32_t* cand_keys, const int* cand_count, int n_img, int cand_cap, int H, int W,
                               int grid_row, int grid_col, int per_cell, int max_kp, uint32_t* kp_keys, int* kp_count,
                               void* stream) {
  VUS_REQUIRE(cand_keys && cand_count && kp_keys && kp_count, "null buffer");
  VUS_REQUIRE(n_img >= 0 && cand_cap >= 1 && max_kp >= 1, "n_img=%d cand_cap=%d max_kp=%d", n_img, cand_cap, max_kp);
  VUS_REQUIRE(H >= 1 && W >= 1 && H < 32768 && W < 32768, "H=%d W=%d", H, W);
  VUS_REQUIRE(grid_row >= 1 && grid_col >= 1 && grid_row <= 256 && grid_col <= 256 && per_cell >= 1,
              "grid %dx%d per_cell=%d", grid_row, grid_col, per_cell);
  if (n_img == 0) return VUS_OK;
  select_grid_kernel<<<n_img, SEL_THREADS, 0, vus::as_stream(stream)>>>(cand_keys, cand_count, cand_cap, H, W, grid_row,
                                                                        grid_col, per_cell, max_kp, kp_keys, kp_count);
  VUS_CHECK_LAUNCH("select_grid");
  return VUS_OK;
}
