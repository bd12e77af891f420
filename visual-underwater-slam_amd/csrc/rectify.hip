// rectify.hip -- vus_rectify_plan / vus_rectify_remap (include/vus_rectify.h): lens undistortion + stereo rectification
// of raw images by a Q5 relative remap table, in front of the detector.  Integer arithmetic only; the header states it.
#include "vus_common.h"
#include <climits>
#include "../../include/vus_rectify.h"

namespace {

constexpr int RCT_THREADS = 256;
constexpr int RCT_TW = VUS_RECTIFY_TILE_W, RCT_TH = VUS_RECTIFY_TILE_H;
constexpr int RCT_PX = 4;                          // consecutive output pixels of a thread
constexpr int RCT_GROUP = VUS_RECTIFY_FRAME_GROUP;
constexpr int RCT_SLOTS = RCT_THREADS / 32;        // images staged side by side: one per 32 lanes
constexpr int RCT_ROWS = 8;                        // box rows a lane has in flight
constexpr int RCT_LDS_DW = 2 * VUS_RECTIFY_LDS_BYTES / 4;   // the LDS array: two boxes of the largest size, 8 lens boxes
static_assert(RCT_TW * RCT_TH == RCT_THREADS * RCT_PX, "a thread owns 4 pixels of the tile");
static_assert(RCT_TW % RCT_PX == 0 && VUS_RECTIFY_LDS_BYTES % 4 == 0, "tile rows are whole threads, the box is dwords");

// what the host found out about the pointers: the wide forms need their alignment
constexpr int RCT_MAP_X4 = 1;   // map rows are 16-byte aligned: one dwordx4 load per thread
constexpr int RCT_DST_DW = 4;   // destination rows are 4-byte aligned: one dword store per thread

// the clamped source pixels and weights of output pixel (x, y): the REMAP statement of the header
struct RctTap {
  int x0, x1, y0, y1, fx, fy;
};

__device__ __forceinline__ RctTap rct_decode(int32_t word, int x, int y, int W, int H) {
  const int dx = (int)(int16_t)(word & 0xFFFF), dy = word >> 16;
  const int sx = (x << 5) + dx, sy = (y << 5) + dy;
  const int ix = sx >> 5, iy = sy >> 5;
  RctTap t;
  t.fx = sx & 31;
  t.fy = sy & 31;
  t.x0 = min(max(ix, 0), W - 1);
  t.x1 = min(max(ix + 1, 0), W - 1);
  t.y0 = min(max(iy, 0), H - 1);
  t.y1 = min(max(iy + 1, 0), H - 1);
  return t;
}

// the 4 map words of this thread (tile column 4 * (tid & 15), tile row tid >> 4); `valid`: bit j = pixel j is in the image
__device__ __forceinline__ int rct_load_words(const int32_t* __restrict__ map_m, int x, int y, int H, int W, bool x4,
                                              int32_t (&w)[RCT_PX]) {
  int valid = 0;
#pragma unroll
  for (int j = 0; j < RCT_PX; ++j) {
    w[j] = 0;
    valid |= (y < H && x + j < W) ? 1 << j : 0;
  }
  if (valid == 0) return 0;
  const int32_t* p = map_m + (size_t)y * W + x;
  if (x4) {   // W is a multiple of 4: all four pixels are inside
    const int4 v = *reinterpret_cast<const int4*>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < RCT_PX; ++j)
      if (valid >> j & 1) w[j] = p[j];
  }
  return valid;
}

// One workgroup per tile and map: the bounding box of the tile's clamped source pixels.
__global__ __launch_bounds__(RCT_THREADS) void rectify_plan_kernel(const int32_t* __restrict__ map, int H, int W,
                                                                   int tiles_x, int n_tiles, int flags,
                                                                   int32_t* __restrict__ boxes) {
  __shared__ int s_red[4][RCT_THREADS / 64];
  const int tile = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * RCT_TW + (tid & 15) * RCT_PX, y = ty * RCT_TH + (tid >> 4);
  int32_t w[RCT_PX];
  const int valid = rct_load_words(map + (size_t)m * H * W, x, y, H, W, flags & RCT_MAP_X4, w);
  int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
#pragma unroll
  for (int j = 0; j < RCT_PX; ++j)
    if (valid >> j & 1) {
      const RctTap t = rct_decode(w[j], x + j, y, W, H);
      xmin = min(xmin, t.x0);
      xmax = max(xmax, t.x1);
      ymin = min(ymin, t.y0);
      ymax = max(ymax, t.y1);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = min(xmin, __shfl_xor(xmin, o));
    ymin = min(ymin, __shfl_xor(ymin, o));
    xmax = max(xmax, __shfl_xor(xmax, o));
    ymax = max(ymax, __shfl_xor(ymax, o));
  }
  if ((tid & 63) == 0) {
    s_red[0][tid >> 6] = xmin;
    s_red[1][tid >> 6] = ymin;
    s_red[2][tid >> 6] = xmax;
    s_red[3][tid >> 6] = ymax;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < RCT_THREADS / 64; ++v) {
      xmin = min(xmin, s_red[0][v]);
      ymin = min(ymin, s_red[1][v]);
      xmax = max(xmax, s_red[2][v]);
      ymax = max(ymax, s_red[3][v]);
    }
    // the tile's first pixel is inside the image: the box is never empty
    const int bw = xmax - xmin + 1, bh = ymax - ymin + 1;
    const bool fits = ((bw + 6) & ~3) * bh <= VUS_RECTIFY_LDS_BYTES;     // < 2^30: bw, bh <= 32767
    reinterpret_cast<int4*>(boxes)[(size_t)m * n_tiles + tile] = fits ? make_int4(xmin, ymin, bw, bh) : make_int4(0, 0, 0, 0);
  }
}

// One output pixel from the rows at p[o0] (y0) and p[o1] (y1), columns x0 and x0 + bx; pk = bx | fx << 1 | fy << 6.
// 32 p00 + fx (p01 - p00) = p00 (32 - fx) + p01 fx, and the same once more down the column: the header's sum exactly.
// pk goes through an empty asm so that its fields are unpacked per image (3 instructions) instead of living in 12
// more registers for the whole group -- with them the kernel was allocated 96 registers: 5 waves per SIMD, not 8.
__device__ __forceinline__ uint32_t rct_pixel(const uint8_t* p, uint32_t o0, uint32_t o1, int pk) {
  asm volatile("" : "+v"(pk));
  const uint32_t bx = pk & 1;
  const int fx = (pk >> 1) & 31, fy = (pk >> 6) & 31;
  const int p00 = p[o0], p01 = p[o0 + bx], p10 = p[o1], p11 = p[o1 + bx];
  const int top = (p00 << 5) + fx * (p01 - p00), bot = (p10 << 5) + fx * (p11 - p10);
  return (uint32_t)((top << 5) + fy * (bot - top) + 512) >> 10;
}

__device__ __forceinline__ void rct_store(uint8_t* __restrict__ d, uint32_t word, int valid, bool dw) {
  if (dw && valid == 15) {
    *reinterpret_cast<uint32_t*>(d) = word;
  } else {
#pragma unroll
    for (int j = 0; j < RCT_PX; ++j)
      if (valid >> j & 1) d[j] = (uint8_t)(word >> (8 * j));
  }
}

// One workgroup per tile, group of images and map.  SRC_DW: source rows are 4-byte aligned and the box is staged as
// dwords; the bytewise form is an instantiation of its own because its loop costs the common one 30 registers.
template <bool SRC_DW>
__global__ __launch_bounds__(RCT_THREADS) void rectify_remap_kernel(
    const uint8_t* __restrict__ src, int n_img, int H, int W, int pitch_s, const int32_t* __restrict__ map,
    const int32_t* __restrict__ boxes, int n_maps, uint8_t* __restrict__ dst, int pitch_d, int tiles_x, int n_tiles,
    int flags) {
  __shared__ uint32_t s_box[RCT_LDS_DW];
  const int tile = blockIdx.x, m = blockIdx.z, tid = threadIdx.x;
  // images m, m + n_maps, ...: numbers k_lo .. k_hi - 1 of them are this workgroup's
  const int n_mine = m < n_img ? (n_img - m + n_maps - 1) / n_maps : 0;
  const int k_lo = blockIdx.y * RCT_GROUP, k_hi = min(n_mine, k_lo + RCT_GROUP);
  if (k_lo >= k_hi) return;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * RCT_TW + (tid & 15) * RCT_PX, y = ty * RCT_TH + (tid >> 4);
  int32_t w[RCT_PX];
  const int valid = rct_load_words(map + (size_t)m * H * W, x, y, H, W, flags & RCT_MAP_X4, w);
  RctTap t[RCT_PX];
#pragma unroll
  for (int j = 0; j < RCT_PX; ++j) t[j] = rct_decode(w[j], min(x + j, W - 1), min(y, H - 1), W, H);

  // the box is a schedule: it is used only if it is what the header says it is
  const int4 box = reinterpret_cast<const int4*>(boxes)[(size_t)m * n_tiles + tile];
  bool staged = box.z >= 1 && box.w >= 1 && box.x >= 0 && box.y >= 0 && box.z <= W - box.x && box.w <= H - box.y &&
                ((box.z + 6) & ~3) * box.w <= VUS_RECTIFY_LDS_BYTES;
  if (staged) {   // workgroup-uniform
    bool inside = true;
#pragma unroll
    for (int j = 0; j < RCT_PX; ++j)
      if (valid >> j & 1)
        inside = inside && t[j].x0 >= box.x && t[j].x1 < box.x + box.z && t[j].y0 >= box.y && t[j].y1 < box.y + box.w;
    staged = __syncthreads_and(inside);
  }

  // per pixel: offsets of the y0 and y1 rows' x0 byte in the staged box or in the image, and the packed rest
  const int xa = box.x & ~3;                               // the staged rows start at an aligned column
  const int stride = staged ? (box.z + 6) & ~3 : pitch_s;
  uint32_t o0[RCT_PX], o1[RCT_PX];
  int pk[RCT_PX];
#pragma unroll
  for (int j = 0; j < RCT_PX; ++j) {
    const bool v = valid >> j & 1;      // a pixel outside the image reads the first byte: in range on either path
    const int col = staged ? t[j].x0 - xa : t[j].x0, r0 = staged ? t[j].y0 - box.y : t[j].y0;
    o0[j] = v ? (uint32_t)(r0 * stride + col) : 0u;
    o1[j] = v ? (uint32_t)((r0 + (t[j].y1 - t[j].y0)) * stride + col) : 0u;
    pk[j] = v ? (t[j].x1 - t[j].x0) | t[j].fx << 1 | t[j].fy << 6 : 0;
  }
  const bool dst_dw = flags & RCT_DST_DW;
  const size_t img_s = (size_t)H * pitch_s, img_d = (size_t)H * pitch_d;
  const size_t out_off = (size_t)min(y, H - 1) * pitch_d + x;

  if (staged) {
    // The boxes of as many images as the LDS array holds (at least 2, 8 for a lens box) are staged side by side: one
    // image per 32 lanes, 32 lanes along a row, 8 rows in flight per lane, so a pass keeps ~11 KB of loads in flight per
    // workgroup.  With one 1.4 KB box per barrier pair 1000 stereo frames of 720p took 2.33 ms, this way 1.44 (both at
    // a frame group of 8; profiles/rectify.md).
    const int ndw = ((box.x & 3) + box.z + 3) >> 2, nb = (box.x & 3) + box.z, s4 = stride >> 2;
    const int box_dw = s4 * box.w, slots = min(RCT_SLOTS, RCT_LDS_DW / box_dw);
    const int slot = tid >> 5, lane = tid & 31;
    for (int k = k_lo; k < k_hi; k += slots) {
      const int nf = min(slots, k_hi - k);
      if (slot < nf) {
        const uint8_t* img = src + ((size_t)m + (size_t)(k + slot) * n_maps) * img_s + (size_t)box.y * pitch_s + xa;
        uint32_t* sb = s_box + slot * box_dw;
        if (SRC_DW) {
          for (int c = lane; c < ndw; c += 32)
            for (int r0 = 0; r0 < box.w; r0 += RCT_ROWS) {
              uint32_t v[RCT_ROWS];      // rows past the box repeat its last row: no branch around a load
#pragma unroll
              for (int u = 0; u < RCT_ROWS; ++u)
                v[u] = *reinterpret_cast<const uint32_t*>(img + (uint32_t)(min(r0 + u, box.w - 1) * pitch_s + 4 * c));
#pragma unroll
              for (int u = 0; u < RCT_ROWS; ++u) sb[min(r0 + u, box.w - 1) * s4 + c] = v[u];
            }
        } else {
          uint8_t* sbb = reinterpret_cast<uint8_t*>(sb);   // the rare form: kept small
#pragma unroll 1
          for (int r = 0; r < box.w; ++r) {
#pragma unroll 1
            for (int c = lane; c < nb; c += 32) sbb[r * stride + c] = img[(uint32_t)(r * pitch_s + c)];
          }
        }
      }
      __syncthreads();
      for (int f = 0; f < nf; ++f) {
        const uint8_t* lds = reinterpret_cast<const uint8_t*>(s_box + f * box_dw);
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < RCT_PX; ++j) word |= rct_pixel(lds, o0[j], o1[j], pk[j]) << (8 * j);
        if (valid) rct_store(dst + ((size_t)m + (size_t)(k + f) * n_maps) * img_d + out_off, word, valid, dst_dw);
      }
      if (k + slots < k_hi) __syncthreads();     // the next pass overwrites the boxes
    }
  } else {
    for (int k = k_lo; k < k_hi; ++k) {
      const size_t i = (size_t)m + (size_t)k * n_maps;
      const uint8_t* img = src + i * img_s;
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < RCT_PX; ++j) word |= rct_pixel(img, o0[j], o1[j], pk[j]) << (8 * j);
      if (valid) rct_store(dst + i * img_d + out_off, word, valid, dst_dw);
    }
  }
}

int rct_check_shape(const char* who, int n_maps, int H, int W) {
  VUS_REQUIRE(n_maps >= 1 && n_maps <= 65535, "%s: n_maps=%d outside 1..65535", who, n_maps);
  VUS_REQUIRE(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "%s: H=%d W=%d outside 1..32767", who, H, W);
  return VUS_OK;
}

inline bool rct_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" int vus_rectify_plan(const int32_t* map, int n_maps, int H, int W, int32_t* boxes, void* stream) {
  VUS_REQUIRE(map && boxes, "null buffer");
  if (int rc = rct_check_shape("rectify_plan", n_maps, H, W)) return rc;
  VUS_REQUIRE(rct_aligned(boxes, 16), "rectify_plan: boxes must be 16-byte aligned");
  const int tiles_x = cdiv(W, RCT_TW), n_tiles = tiles_x * cdiv(H, RCT_TH);
  const int flags = (W % 4 == 0 && rct_aligned(map, 16)) ? RCT_MAP_X4 : 0;
  rectify_plan_kernel<<<dim3(n_tiles, n_maps), RCT_THREADS, 0, vus::as_stream(stream)>>>(map, H, W, tiles_x, n_tiles, flags,
                                                                                          boxes);
  VUS_CHECK_LAUNCH("rectify_plan");
  return VUS_OK;
}

extern "C" int vus_rectify_remap(const uint8_t* src, int n_img, int H, int W, int pitch_s, const int32_t* map,
                                 const int32_t* boxes, int n_maps, uint8_t* dst, int pitch_d, void* stream) {
  VUS_REQUIRE(src && map && boxes && dst, "null buffer");
  if (int rc = rct_check_shape("rectify_remap", n_maps, H, W)) return rc;
  VUS_REQUIRE(n_img >= 1, "rectify_remap: n_img=%d, needs at least one image", n_img);
  VUS_REQUIRE(pitch_s >= W && pitch_d >= W, "rectify_remap: pitch_s=%d pitch_d=%d below W=%d", pitch_s, pitch_d, W);
  VUS_REQUIRE((long long)H * pitch_s <= INT_MAX && (long long)H * pitch_d <= INT_MAX,
              "rectify_remap: an image of H=%d rows of pitch %d / %d exceeds 2^31 bytes", H, pitch_s, pitch_d);
  VUS_REQUIRE(rct_aligned(boxes, 16), "rectify_remap: boxes must be 16-byte aligned");
  const int groups = cdiv(cdiv(n_img, n_maps), RCT_GROUP);
  VUS_REQUIRE(groups <= 65535, "rectify_remap: n_img=%d over n_maps=%d is more than %d images per map", n_img, n_maps,
              65535 * RCT_GROUP);
  const int tiles_x = cdiv(W, RCT_TW), n_tiles = tiles_x * cdiv(H, RCT_TH);
  int flags = 0;
  if (W % 4 == 0 && rct_aligned(map, 16)) flags |= RCT_MAP_X4;
  if (pitch_d % 4 == 0 && rct_aligned(dst, 4)) flags |= RCT_DST_DW;
  const dim3 grid(n_tiles, groups, n_maps);
  if (pitch_s % 4 == 0 && rct_aligned(src, 4))
    rectify_remap_kernel<true><<<grid, RCT_THREADS, 0, vus::as_stream(stream)>>>(src, n_img, H, W, pitch_s, map, boxes, n_maps,
                                                                                 dst, pitch_d, tiles_x, n_tiles, flags);
  else
    rectify_remap_kernel<false><<<grid, RCT_THREADS, 0, vus::as_stream(stream)>>>(src, n_img, H, W, pitch_s, map, boxes, n_maps,
                                                                                  dst, pitch_d, tiles_x, n_tiles, flags);
  VUS_CHECK_LAUNCH("rectify_remap");
  return VUS_OK;
}
