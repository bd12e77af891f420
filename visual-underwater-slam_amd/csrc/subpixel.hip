// subpixel.hip -- vus_stereo_refine (include/vus_subpixel.h): an integer SAD search around every stereo match and the
// equiangular fit of its minimum, in 1/256 px.  Integer arithmetic throughout: every output word equals the numpy statement
// of the test suite (tests/subpixel_ref.py).
#include "vus_common.h"
#include "../../include/vus_subpixel.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_LANES = 16;                                   // lanes per slot: lane r owns window row r
constexpr int SP_SLOTS = SP_THREADS / SP_LANES;                // slots per workgroup
constexpr int SP_ROW = 2 * VUS_SUBPIX_MAX_HALF_WIN + 1;        // 15 bytes of a left row at most
constexpr int SP_STRIP = SP_ROW + 2 * VUS_SUBPIX_MAX_SEARCH;   // 31 bytes of a right strip at most
constexpr int SP_SHIFTS = 2 * VUS_SUBPIX_MAX_SEARCH + 1;       // 17 shifts at most
constexpr int SP_LW = (SP_ROW + 3) / 4;                        // 4 registers hold a left row
constexpr int SP_RW = (SP_STRIP + 3) / 4 + 1;                  // 8 hold a strip; one more (zero) feeds the last byte-align
constexpr int SP_PK = (SP_SHIFTS + 1) / 2;                     // partial sums travel two to a register
static_assert(SP_ROW <= SP_LANES, "one lane per window row");
static_assert(255 * SP_ROW * SP_ROW < 65536, "a cost fits 16 bits");
static_assert((SP_SHIFTS - 1) / 4 + SP_LW < SP_RW, "the last shift's last byte-align stays inside the strip registers");

// One slot per 16 lanes.  The loops run to the compile-time maxima with uniform guards, so every register array is
// indexed by constants (nothing goes to scratch); half_win and search are the same for the whole grid.
__global__ __launch_bounds__(SP_THREADS) void stereo_refine_kernel(
    const uint8_t* __restrict__ img, int H, int W, int pitch, const int32_t* __restrict__ stereo_idx,
    const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count, int max_kp, int total, int half_win, int search,
    int32_t* __restrict__ disp_q8, uint8_t* __restrict__ status) {
  const int r = threadIdx.x & (SP_LANES - 1);
  const int slot = blockIdx.x * SP_SLOTS + (threadIdx.x >> 4);
  if (slot >= total) return;                                   // whole 16-lane groups leave together, here and below
  const int f = slot / max_kp, i = slot - f * max_kp;
  const int nl = min(kp_count[2 * f], max_kp), nr = min(kp_count[2 * f + 1], max_kp);   // a negative count: no keypoint
  int j = -1;
  if (i < nl) j = stereo_idx[slot];
  if (!(i < nl && j >= 0 && j < nr)) {
    if (r == 0) {
      disp_q8[slot] = 0;
      status[slot] = VUS_SUBPIX_NONE;
    }
    return;
  }
  const uint32_t p = kp_keys[(size_t)(2 * f) * max_kp + i] & VUS_KEY_POS_MASK;
  const uint32_t q = kp_keys[(size_t)(2 * f + 1) * max_kp + j] & VUS_KEY_POS_MASK;
  const int yl = (int)(p / (uint32_t)W), xl = (int)(p - (uint32_t)yl * (uint32_t)W), xr = (int)(q - (q / (uint32_t)W) * (uint32_t)W);
  const int win = 2 * half_win + 1, strip = win + 2 * search, shifts = 2 * search + 1;

  // lane r: row r of the left window and of the right strip, four bytes to a register
  uint32_t Lw[SP_LW], Rw[SP_RW];
#pragma unroll
  for (int k = 0; k < SP_LW; ++k) Lw[k] = 0u;
#pragma unroll
  for (int k = 0; k < SP_RW; ++k) Rw[k] = 0u;
  // bytes of a shifted strip past the window's width do not count (the left row holds zeros there)
  uint32_t mask[SP_LW];
#pragma unroll
  for (int k = 0; k < SP_LW; ++k) {
    const int n = min(max(win - 4 * k, 0), 4);
    mask[k] = n == 4 ? 0xFFFFFFFFu : ((1u << (8 * n)) - 1u);
  }
  if (r < win) {
    const int y = min(max(yl + r - half_win, 0), H - 1);
    const uint8_t* lrow = img + ((size_t)(2 * f) * H + y) * pitch;
    const uint8_t* rrow = lrow + (size_t)H * pitch;
    const int x0l = xl - half_win, x0r = xr - search - half_win;
    // a row whose whole-dword span lies inside the W pixels of its image row needs no clamp: unaligned dword loads (2.7x
    // faster than byte loads at an 11 x 11 window on the MI355X, profiles/subpixel.md); any other row: clamped byte loads
    const int ndl = (win + 3) >> 2, ndr = (strip + 3) >> 2;
    if (x0l >= 0 && x0l + 4 * ndl <= W) {
#pragma unroll
      for (int k = 0; k < SP_LW; ++k)
        if (k < ndl) {
          uint32_t v;
          __builtin_memcpy(&v, lrow + x0l + 4 * k, 4);
          Lw[k] = v & mask[k];
        }
    } else {
#pragma unroll
      for (int b = 0; b < SP_ROW; ++b)
        if (b < win) {
          const int x = min(max(x0l + b, 0), W - 1);
          Lw[b >> 2] |= (uint32_t)lrow[x] << (8 * (b & 3));
        }
    }
    if (x0r >= 0 && x0r + 4 * ndr <= W) {
#pragma unroll
      for (int k = 0; k < SP_RW - 1; ++k)
        if (k < ndr) {
          uint32_t v;
          __builtin_memcpy(&v, rrow + x0r + 4 * k, 4);
          Rw[k] = v;                           // bytes past the strip are never inside a masked window
        }
    } else {
#pragma unroll
      for (int b = 0; b < SP_STRIP; ++b)
        if (b < strip) {
          const int x = min(max(x0r + b, 0), W - 1);
          Rw[b >> 2] |= (uint32_t)rrow[x] << (8 * (b & 3));
        }
    }
  }
  // this row's share of cost(s - search); a lane without a row holds zeros and adds nothing
  uint32_t c[2 * SP_PK];
#pragma unroll
  for (int s = SP_SHIFTS; s < 2 * SP_PK; ++s) c[s] = 0u;
#pragma unroll
  for (int s = 0; s < SP_SHIFTS; ++s) {
    uint32_t acc = 0u;
    if (s < shifts) {
#pragma unroll
      for (int k = 0; k < SP_LW; ++k) {
        const uint32_t w = __builtin_amdgcn_alignbyte(Rw[s / 4 + k + 1], Rw[s / 4 + k], (uint32_t)(s & 3));
        acc = __builtin_amdgcn_sad_u8(Lw[k], w & mask[k], acc);
      }
    }
    c[s] = acc;
  }
  // the 16 rows added: two 16-bit sums per register (a full cost is at most 57375)
  uint32_t pk[SP_PK];
#pragma unroll
  for (int k = 0; k < SP_PK; ++k) pk[k] = c[2 * k] | (c[2 * k + 1] << 16);
#pragma unroll
  for (int o = SP_LANES / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < SP_PK; ++k) pk[k] += (uint32_t)__shfl_xor((int)pk[k], o, SP_LANES);
  }
  if (r != 0) return;
#pragma unroll
  for (int k = 0; k < SP_PK; ++k) {
    c[2 * k] = pk[k] & 0xFFFFu;
    c[2 * k + 1] = pk[k] >> 16;
  }
  uint32_t c0 = c[0];
  int sb = 0;
#pragma unroll
  for (int s = 1; s < SP_SHIFTS; ++s)
    if (s < shifts && c[s] < c0) {                               // strict: the lowest s wins a tie
      c0 = c[s];
      sb = s;
    }
  const uint32_t d0 = (uint32_t)(xl - xr);                       // unsigned from here on: wraps like the int32 statement
  uint32_t dq = 256u * d0;
  uint8_t st = VUS_SUBPIX_EDGE;
  if (sb > 0 && sb < shifts - 1) {
    uint32_t cm = 0u, cp = 0u;
#pragma unroll
    for (int s = 0; s < SP_SHIFTS; ++s) {
      if (s == sb - 1) cm = c[s];
      if (s == sb + 1) cp = c[s];
    }
    const uint32_t m = max(cm, cp) - c0;
    int fit = 0;
    // floor((256 (cm - cp) + m) / (2 m)): |cm - cp| <= m, so adding 128 (2 m) makes the numerator positive
    if (m > 0u) fit = (int)((256u * cm - 256u * cp + 257u * m) / (2u * m)) - 128;
    dq = 256u * (d0 - (uint32_t)(sb - search)) - (uint32_t)fit;
    st = VUS_SUBPIX_OK;
  }
  disp_q8[slot] = (int32_t)dq;
  status[slot] = st;
}

}  // namespace

extern "C" int vus_stereo_refine(const uint8_t* img, int n_frames, int H, int W, int pitch, const int32_t* stereo_idx,
                                 const uint32_t* kp_keys, const int* kp_count, int max_kp, int half_win, int search,
                                 int32_t* disp_q8, uint8_t* status, void* stream) {
  VUS_REQUIRE(img, "stereo_refine: img is null");
  VUS_REQUIRE(stereo_idx, "stereo_refine: stereo_idx is null");
  VUS_REQUIRE(kp_keys, "stereo_refine: kp_keys is null");
  VUS_REQUIRE(kp_count, "stereo_refine: kp_count is null");
  VUS_REQUIRE(disp_q8, "stereo_refine: disp_q8 is null");
  VUS_REQUIRE(status, "stereo_refine: status is null");
  VUS_REQUIRE(n_frames >= 1, "stereo_refine: n_frames=%d, needs at least one frame", n_frames);
  VUS_REQUIRE(H >= 1, "stereo_refine: H=%d", H);
  VUS_REQUIRE(W >= 1, "stereo_refine: W=%d", W);
  VUS_REQUIRE(pitch >= W, "stereo_refine: pitch=%d below W=%d", pitch, W);
  VUS_REQUIRE(max_kp >= 1 && max_kp <= 65535, "stereo_refine: max_kp=%d outside 1..65535", max_kp);
  VUS_REQUIRE(half_win >= 1 && half_win <= VUS_SUBPIX_MAX_HALF_WIN, "stereo_refine: half_win=%d outside 1..%d", half_win,
              VUS_SUBPIX_MAX_HALF_WIN);
  VUS_REQUIRE(search >= 1 && search <= VUS_SUBPIX_MAX_SEARCH, "stereo_refine: search=%d outside 1..%d", search,
              VUS_SUBPIX_MAX_SEARCH);
  const long long total = (long long)n_frames * max_kp;
  VUS_REQUIRE(total < (1ll << 31), "stereo_refine: n_frames=%d times max_kp=%d overflows the int32 slot index", n_frames, max_kp);
  VUS_REQUIRE((long long)H * pitch < (1ll << 31), "stereo_refine: an image plane of H=%d rows of pitch=%d bytes is 2 GiB or more",
              H, pitch);
  stereo_refine_kernel<<<cdiv(total, SP_SLOTS), SP_THREADS, 0, vus::as_stream(stream)>>>(
      img, H, W, pitch, stereo_idx, kp_keys, kp_count, max_kp, (int)total, half_win, search, disp_q8, status);
  VUS_CHECK_LAUNCH("stereo_refine");
  return VUS_OK;
}
