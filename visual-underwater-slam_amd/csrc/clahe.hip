// clahe.hip -- vus_clahe_luts / vus_clahe_apply (include/vus_clahe.h): contrast-limited adaptive histogram equalisation
// of 8-bit images in front of the detector.  Integer arithmetic only; the header states it.
#include "vus_common.h"
#include <climits>
#include "../../include/vus_clahe.h"

namespace {

constexpr int CLH_THREADS = 256;
constexpr int CLH_PX = 4;                          // pixels of a thread of the apply kernel: one dword
constexpr int CLH_COPIES = VUS_CLAHE_HIST_COPIES;  // interleaved histograms: bin b of copy c is dword b * CLH_COPIES + c
constexpr int CLH_LOADS = 4;                       // loads a thread has in flight
constexpr int CLH_ROWS = CLH_THREADS;              // rows of a cell whose weights are staged at a time
static_assert(CLH_COPIES >= 1 && CLH_COPIES <= 32 && (CLH_COPIES & (CLH_COPIES - 1)) == 0, "a copy per lane of a half wave at most");

// what the host found out about the pointers: the wide forms need their alignment
constexpr int CLH_LUT_DW = 1;   // luts is 4-byte aligned: a lane writes its 4 bins as one dword
constexpr int CLH_DST_DW = 2;   // destination rows are 4-byte aligned: one dword store per thread

// VEC consecutive bytes of a row, as dwords: 16 (rows 16-byte aligned), 4 (4-byte aligned) or 1
template <int VEC>
__device__ __forceinline__ void clh_load(const uint8_t* q, uint32_t (&v)[(VEC + 3) / 4]) {
  if constexpr (VEC == 16) {
    const uint4 t = *reinterpret_cast<const uint4*>(q);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (VEC == 4) {
    v[0] = *reinterpret_cast<const uint32_t*>(q);
  } else {
    v[0] = *q;
  }
}

// Which cell of which image workgroup (blockIdx.x, blockIdx.y) of the apply kernel takes, as (cell, first image).
// Neighbouring cells of an image share 128-byte lines (a 720p cell row is 160 bytes from a multiple of 80), and consecutive
// workgroups go to different XCDs, each with an L2 of its own: so the grid is dealt out in eight contiguous runs, one per
// residue of the workgroup number mod 8, and the cells of one image stay on one L2 (apply 1.10 -> 0.94 ms; the table kernel,
// which only reads, gained nothing and keeps its block indices).  A placement guess: it changes speed only.
__device__ __forceinline__ void clh_piece(int* piece, int* first) {
  const uint32_t n = gridDim.x * gridDim.y, id = blockIdx.x + gridDim.x * blockIdx.y;     // n <= 1089 * 65535
  const uint32_t q = n >> 3, rem = n & 7, g = id & 7, pos = id >> 3;
  const uint32_t v = (g < rem ? g * (q + 1) : rem * (q + 1) + (g - rem) * q) + pos;
  *first = (int)(v / gridDim.x);
  *piece = (int)(v - (uint32_t)*first * gridDim.x);
}

__device__ __forceinline__ int clh_wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

__device__ __forceinline__ int clh_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Adds columns [x_lo, x_hi) (non-empty, inside the image) of the source rows of padded rows row0 .. row0 + th - 1 to the
// histogram copy at `mine`.  Rows are VEC-byte aligned and an item is the aligned vector at column a_lo + VEC k, of which
// the bytes outside the span are skipped (x_hi rounded up to VEC is at most the pitch: no vector leaves its row).  Items
// are dealt to the threads round robin; a thread follows its (row, k) by additions, so nothing is divided per item.
template <int VEC>
__device__ __forceinline__ void clh_count_span(const uint8_t* img, int pitch, int H, int row0, int th, int x_lo, int x_hi,
                                               uint32_t* mine) {
  const int tid = threadIdx.x;
  constexpr int NW = (VEC + 3) / 4;
  const int a_lo = x_lo & ~(VEC - 1);
  const int per_row = (x_hi - a_lo + VEC - 1) / VEC;
  const int n_items = th * per_row;                       // <= T <= 2^22
  const int d_rr = CLH_THREADS / per_row, d_k = CLH_THREADS - d_rr * per_row;
  int rr = tid / per_row, k = tid - rr * per_row;
  for (int item = tid; item < n_items; item += CLH_LOADS * CLH_THREADS) {
    uint32_t v[CLH_LOADS][NW];
    int col[CLH_LOADS];
#pragma unroll
    for (int u = 0; u < CLH_LOADS; ++u) {
      const bool on = item + u * CLH_THREADS < n_items;   // then rr < th
      const int p = row0 + rr, sr = p < H ? p : 2 * (H - 1) - p;
      const int c = a_lo + VEC * k;
      col[u] = on ? c : x_hi;                             // an item past the end owns no column
#pragma unroll
      for (int w = 0; w < NW; ++w) v[u][w] = 0;
      if (on) clh_load<VEC>(img + (uint32_t)(sr * pitch + c), v[u]);
      k += d_k;
      rr += d_rr;
      if (k >= per_row) {
        k -= per_row;
        ++rr;
      }
    }
#pragma unroll
    for (int u = 0; u < CLH_LOADS; ++u) {
      if (col[u] >= x_lo && col[u] + VEC <= x_hi) {       // a whole vector, the common case: no test per byte
#pragma unroll
        for (int b = 0; b < VEC; ++b) atomicAdd(&mine[((v[u][b >> 2] >> (8 * (b & 3))) & 255u) * CLH_COPIES], 1u);
      } else {
#pragma unroll
        for (int b = 0; b < VEC; ++b)
          if (col[u] + b >= x_lo && col[u] + b < x_hi) atomicAdd(&mine[((v[u][b >> 2] >> (8 * (b & 3))) & 255u) * CLH_COPIES], 1u);
      }
    }
  }
}

// One workgroup per tile and image; past 65535 images blockIdx.y strides over them.
template <int VEC>
__global__ __launch_bounds__(CLH_THREADS) void clahe_lut_kernel(const uint8_t* __restrict__ src, int n_img, int H, int W,
                                                                 int pitch, int tiles_x, int tw, int th, int clip,
                                                                 uint8_t* __restrict__ luts, int flags) {
  __shared__ uint32_t s_hist[256 * CLH_COPIES];
  __shared__ uint32_t s_tot[256];
  const int tile = blockIdx.x, n_tiles = gridDim.x, tid = threadIdx.x;
  const int j = tile / tiles_x, i = tile - j * tiles_x;
  const int c0 = i * tw, row0 = j * th, T = tw * th;
  // the tile's columns inside the image, and the image columns its padded columns max(c0, W) .. c0 + tw - 1 reflect to
  const int a_lo = c0, a_hi = min(c0 + tw, W);
  const int b_lo = 2 * W - 1 - c0 - tw, b_hi = 2 * W - 1 - max(c0, W);     // b_lo >= 0: tiles_x tw <= 2 W - 1
  uint32_t* mine = s_hist + (tid & (CLH_COPIES - 1));
  for (int img = blockIdx.y; img < n_img; img += gridDim.y) {
    const uint8_t* im = src + (size_t)img * H * pitch;
    for (int e = tid; e < 256 * CLH_COPIES; e += CLH_THREADS) s_hist[e] = 0;
    __syncthreads();
    if (a_hi > a_lo) clh_count_span<VEC>(im, pitch, H, row0, th, a_lo, a_hi, mine);
    if (b_hi > b_lo) clh_count_span<VEC>(im, pitch, H, row0, th, b_lo, b_hi, mine);
    __syncthreads();
    {   // bin tid: its copies, each thread starting at another one so that a half wave reads 32 banks
      uint32_t s = 0;
#pragma unroll
      for (int c = 0; c < CLH_COPIES; ++c) s += s_hist[tid * CLH_COPIES + ((c + tid) & (CLH_COPIES - 1))];
      s_tot[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: bins 4 tid .. 4 tid + 3
      int h[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] = (int)s_tot[4 * tid + q];
      if (clip > 0) {
        int ex = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ex += max(h[q] - clip, 0);
          h[q] = min(h[q], clip);
        }
        ex = clh_wave_sum(ex);
        const int batch = ex >> 8, r = ex & 255, step = r > 0 ? max(256 / r, 1) : 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = 4 * tid + q;
          h[q] += batch + ((r > 0 && b % step == 0 && b / step < r) ? 1 : 0);
        }
      }
      const int own = h[0] + h[1] + h[2] + h[3];
      uint32_t c = (uint32_t)(clh_wave_incl_scan(own) - own), word = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        c += (uint32_t)h[q];
        word |= ((c * 255u + (uint32_t)(T >> 1)) / (uint32_t)T) << (8 * q);     // c <= T <= 2^22: below 2^31
      }
      uint8_t* out = luts + ((size_t)img * n_tiles + tile) * 256 + 4 * tid;
      if (flags & CLH_LUT_DW) {
        *reinterpret_cast<uint32_t*>(out) = word;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = (uint8_t)(word >> (8 * q));
      }
    }
    // the next image's zeroing touches s_hist only, and s_tot is rewritten two barriers later
  }
}

typedef unsigned short clh_u16x2 __attribute__((ext_vector_type(2)));

// weight of position x along an axis with tile size t in the cell whose first tile is t1 = cell - 1
__device__ __forceinline__ int clh_weight(int x, int t, int cell) {
  const int a = 2 * x - t - (cell - 1) * 2 * t;      // in [0, 2 t) for a position inside the cell
  return (a * 256 + t) / (2 * t);
}

// One workgroup per cell (the rectangle between tile centres) and image (clh_piece).  src and dst may be the same buffer:
// a thread writes only bytes it owns, a partial dword bytewise.  A thread owns the CLH_PX pixels of an aligned dword of a
// row; SRC_DW: the source rows are 4-byte aligned and it loads them as one dword.  (16 pixels per thread with 16-byte
// loads and stores took the same time before the XCD placement and 20 % more after it: profiles/clahe.md.)
template <bool SRC_DW>
__global__ __launch_bounds__(CLH_THREADS) void clahe_apply_kernel(const uint8_t* src, int n_img, int H, int W, int pitch_s,
                                                                   const uint8_t* __restrict__ luts, int tiles_x, int tiles_y,
                                                                   int tw, int th, uint8_t* dst, int pitch_d, int flags) {
  __shared__ uint32_t s_lut[256];        // grey level v: lut[y1][x1][v] | lut[y1][x2][v] << 8 | lut[y2][x1][v] << 16 | [y2][x2] << 24
  __shared__ uint32_t s_wy[CLH_ROWS];    // row r of the pass: (256 - wy) | wy << 16
  const int cells_x = tiles_x + 1, tid = threadIdx.x;
  int cell, img0;
  clh_piece(&cell, &img0);
  const int cy = cell / cells_x, cx = cell - cy * cells_x;
  const int hx = (tw + 1) >> 1, hy = (th + 1) >> 1;
  const int x_lo = cx ? hx + (cx - 1) * tw : 0, x_hi = min(W, hx + cx * tw);
  const int y_lo = cy ? hy + (cy - 1) * th : 0, y_hi = min(H, hy + cy * th);
  if (x_lo >= x_hi || y_lo >= y_hi) return;          // a cell beyond the image (the padding holds whole tiles)
  const int tx1 = min(max(cx - 1, 0), tiles_x - 1), tx2 = min(cx, tiles_x - 1);
  const int ty1 = min(max(cy - 1, 0), tiles_y - 1), ty2 = min(cy, tiles_y - 1);
  // threads: lx along the cell's dwords (from the aligned column a_lo), ly along its rows
  const int a_lo = x_lo & ~(CLH_PX - 1), ndw = (x_hi - a_lo + CLH_PX - 1) / CLH_PX;
  const int two_t = 2 * tw, dq = 512 / two_t, dr = 512 - dq * two_t;     // wx of the next column: the quotient grows by 512 / 2 tw
  const int LX = min(ndw, CLH_THREADS), LY = CLH_THREADS / LX;
  const int ly = tid / LX, lx = tid - ly * LX;
  const bool dst_dw = flags & CLH_DST_DW;
  const size_t n_tiles = (size_t)tiles_x * tiles_y;
  for (int img = img0; img < n_img; img += gridDim.y) {
    const uint8_t* im = src + (size_t)img * H * pitch_s;
    uint8_t* om = dst + (size_t)img * H * pitch_d;
    const uint8_t* lt = luts + (size_t)img * n_tiles * 256;
    for (int yc = y_lo; yc < y_hi; yc += CLH_ROWS) {
      const int nr = min(CLH_ROWS, y_hi - yc);
      __syncthreads();                                 // the readers of the previous pass are done
      if (yc == y_lo)
        s_lut[tid] = (uint32_t)lt[(ty1 * tiles_x + tx1) * 256 + tid] | (uint32_t)lt[(ty1 * tiles_x + tx2) * 256 + tid] << 8 |
                     (uint32_t)lt[(ty2 * tiles_x + tx1) * 256 + tid] << 16 | (uint32_t)lt[(ty2 * tiles_x + tx2) * 256 + tid] << 24;
      if (tid < nr) {
        const uint32_t wy = (uint32_t)clh_weight(yc + tid, th, cy);
        s_wy[tid] = (256u - wy) | wy << 16;
      }
      __syncthreads();
      if (ly >= LY) continue;                          // barriers are reached by every thread: this skips the work only
      for (int k = lx; k < ndw; k += LX) {
        const int col = a_lo + CLH_PX * k, first = max(col, x_lo);
        uint32_t wx[CLH_PX], wxc[CLH_PX];              // wx and 256 - wx, each in both halves of a dword
        int valid = 0;
        {   // one division for the thread's first column inside the cell, then exact steps of quotient and remainder
          int q = clh_weight(first, tw, cx), r = (2 * first - tw - (cx - 1) * two_t) * 256 + tw - q * two_t;
#pragma unroll
          for (int b = 0; b < CLH_PX; ++b) {
            const bool in = col + b >= x_lo && col + b < x_hi;
            valid |= in ? 1 << b : 0;
            wx[b] = in ? (uint32_t)q * 0x10001u : 0u;
            wxc[b] = in ? (uint32_t)(256 - q) * 0x10001u : 0u;
            if (col + b >= first) {
              q += dq;
              r += dr;
              if (r >= two_t) {
                r -= two_t;
                ++q;
              }
            }
          }
        }
        for (int r0 = ly; r0 < nr; r0 += CLH_LOADS * LY) {
          uint32_t w[CLH_LOADS];
#pragma unroll
          for (int u = 0; u < CLH_LOADS; ++u) {
            const int r = r0 + u * LY;
            w[u] = 0;
            if (r < nr) {
              const uint8_t* q = im + (uint32_t)((yc + r) * pitch_s + col);
              if (SRC_DW) {
                w[u] = *reinterpret_cast<const uint32_t*>(q);
              } else {
#pragma unroll
                for (int b = 0; b < CLH_PX; ++b)
                  if (valid >> b & 1) w[u] |= (uint32_t)q[b] << (8 * b);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < CLH_LOADS; ++u) {
            const int r = r0 + u * LY;
            if (r >= nr) break;
            const clh_u16x2 wy = __builtin_bit_cast(clh_u16x2, s_wy[r]);
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < CLH_PX; ++b) {
              // the contract's sum in three instructions: the two blends along x as one packed 16-bit multiply-add (each
              // at most 255 * 256), the blend along y and the rounding term as one 16-bit dot product
              const uint32_t L = s_lut[(w[u] >> (8 * b)) & 255u];
              const uint32_t l1 = __builtin_amdgcn_perm(0u, L, 0x0c020c00u);       // [y1][x1] | [y2][x1] << 16
              const uint32_t l2 = __builtin_amdgcn_perm(0u, L, 0x0c030c01u);       // [y1][x2] | [y2][x2] << 16
              const clh_u16x2 tb = __builtin_bit_cast(clh_u16x2, l1) * __builtin_bit_cast(clh_u16x2, wxc[b]) +
                                   __builtin_bit_cast(clh_u16x2, l2) * __builtin_bit_cast(clh_u16x2, wx[b]);
              word |= (__builtin_amdgcn_udot2(tb, wy, 32768u, false) >> 16) << (8 * b);
            }
            uint8_t* d = om + (uint32_t)((yc + r) * pitch_d + col);
            if (dst_dw && valid == 15) {
              *reinterpret_cast<uint32_t*>(d) = word;
            } else {
#pragma unroll
              for (int b = 0; b < CLH_PX; ++b)
                if (valid >> b & 1) d[b] = (uint8_t)(word >> (8 * b));
            }
          }
        }
      }
    }
  }
}

inline bool clh_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// the checks both entry points share; tw and th on success
int clh_check(const char* who, int n_img, int H, int W, int pitch_s, int tiles_x, int tiles_y, int* tw, int* th) {
  VUS_REQUIRE(n_img >= 1, "%s: n_img=%d, needs at least one image", who, n_img);
  VUS_REQUIRE(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "%s: H=%d W=%d outside 1..32767", who, H, W);
  VUS_REQUIRE(pitch_s >= W, "%s: pitch_s=%d below W=%d", who, pitch_s, W);
  VUS_REQUIRE((long long)H * pitch_s <= INT_MAX, "%s: an image of H=%d rows of pitch_s=%d exceeds 2^31 bytes", who, H, pitch_s);
  VUS_REQUIRE(tiles_x >= 1 && tiles_x <= VUS_CLAHE_MAX_TILES && tiles_y >= 1 && tiles_y <= VUS_CLAHE_MAX_TILES,
              "%s: tiles_x=%d tiles_y=%d outside 1..%d", who, tiles_x, tiles_y, VUS_CLAHE_MAX_TILES);
  *tw = cdiv(W, tiles_x);
  *th = cdiv(H, tiles_y);
  VUS_REQUIRE(tiles_y * *th - H <= H - 1, "%s: tiles_y=%d pads H=%d by %d rows, reflect-101 has H - 1 = %d", who, tiles_y, H,
              tiles_y * *th - H, H - 1);
  VUS_REQUIRE(tiles_x * *tw - W <= W - 1, "%s: tiles_x=%d pads W=%d by %d columns, reflect-101 has W - 1 = %d", who, tiles_x, W,
              tiles_x * *tw - W, W - 1);
  VUS_REQUIRE((long long)*tw * *th <= VUS_CLAHE_MAX_TILE_PIXELS, "%s: a tile of T=%lld pixels (%d x %d) exceeds 2^22", who,
              (long long)*tw * *th, *tw, *th);
  return VUS_OK;
}

}  // namespace

extern "C" int vus_clahe_luts(const uint8_t* src, int n_img, int H, int W, int pitch_s, int tiles_x, int tiles_y, int clip,
                              uint8_t* luts, void* stream) {
  VUS_REQUIRE(src && luts, "clahe_luts: null buffer");
  int tw, th;
  if (int rc = clh_check("clahe_luts", n_img, H, W, pitch_s, tiles_x, tiles_y, &tw, &th)) return rc;
  VUS_REQUIRE(clip >= 0, "clahe_luts: clip=%d is negative", clip);
  const int flags = clh_aligned(luts, 4) ? CLH_LUT_DW : 0;
  const dim3 grid(tiles_x * tiles_y, min(n_img, 65535));
  const hipStream_t st = vus::as_stream(stream);
  if (pitch_s % 16 == 0 && clh_aligned(src, 16))
    clahe_lut_kernel<16><<<grid, CLH_THREADS, 0, st>>>(src, n_img, H, W, pitch_s, tiles_x, tw, th, clip, luts, flags);
  else if (pitch_s % 4 == 0 && clh_aligned(src, 4))
    clahe_lut_kernel<4><<<grid, CLH_THREADS, 0, st>>>(src, n_img, H, W, pitch_s, tiles_x, tw, th, clip, luts, flags);
  else
    clahe_lut_kernel<1><<<grid, CLH_THREADS, 0, st>>>(src, n_img, H, W, pitch_s, tiles_x, tw, th, clip, luts, flags);
  VUS_CHECK_LAUNCH("clahe_luts");
  return VUS_OK;
}

extern "C" int vus_clahe_apply(const uint8_t* src, int n_img, int H, int W, int pitch_s, const uint8_t* luts, int tiles_x,
                               int tiles_y, uint8_t* dst, int pitch_d, void* stream) {
  VUS_REQUIRE(src && luts && dst, "clahe_apply: null buffer");
  int tw, th;
  if (int rc = clh_check("clahe_apply", n_img, H, W, pitch_s, tiles_x, tiles_y, &tw, &th)) return rc;
  VUS_REQUIRE(pitch_d >= W, "clahe_apply: pitch_d=%d below W=%d", pitch_d, W);
  VUS_REQUIRE((long long)H * pitch_d <= INT_MAX, "clahe_apply: an image of H=%d rows of pitch_d=%d exceeds 2^31 bytes", H, pitch_d);
  const int flags = (pitch_d % 4 == 0 && clh_aligned(dst, 4)) ? CLH_DST_DW : 0;
  const dim3 grid((tiles_x + 1) * (tiles_y + 1), min(n_img, 65535));
  const hipStream_t st = vus::as_stream(stream);
  if (pitch_s % 4 == 0 && clh_aligned(src, 4))
    clahe_apply_kernel<true><<<grid, CLH_THREADS, 0, st>>>(src, n_img, H, W, pitch_s, luts, tiles_x, tiles_y, tw, th, dst, pitch_d,
                                                           flags);
  else
    clahe_apply_kernel<false><<<grid, CLH_THREADS, 0, st>>>(src, n_img, H, W, pitch_s, luts, tiles_x, tiles_y, tw, th, dst, pitch_d,
                                                            flags);
  VUS_CHECK_LAUNCH("clahe_apply");
  return VUS_OK;
}
