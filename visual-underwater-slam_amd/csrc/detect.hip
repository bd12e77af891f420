// detect.hip -- the detector of the stereo ORB front-end (frontend_common.h): FAST-9/16 + NMS + smoothing, plain and
// adaptive.
//
// Design notes (MI355X):
//  * fast_detect stages a 144x32 byte tile (128x24 outputs + halo) in LDS once, as dwords, and
//    derives score, non-max suppression and the 7x7 smoothing from it: the image is read from HBM
//    once; the score map never goes to HBM (candidates leave the CU as 4-byte keys);
//  * the phases that walk the whole tile work on strips of 4 adjacent pixels read with ds_read_b32/b64
//    and unpacked in registers (SDWA byte selects): byte-wide LDS reads made the first version
//    LDS-issue bound.  The phases that walk a sparse list read the few bytes they need as bytes;
//  * scoring is a two-stage necessary test, then the exact score.  Stage one is per strip, from the
//    (min, max) of every staged dword recorded while staging; stage two is per pixel of the listed
//    strips, on four opposite pairs of the circle (N/S, E/W, the two diagonals).  Survivors are
//    compacted into an LDS work list (DPP wave scan) and the exact score runs on dense lanes, one
//    pixel per lane, from 17 byte reads around the pixel (v_min3/v_max3 sliding windows);
//  * the per-pixel pre-test is two comparisons, one per side (bright arcs, dark arcs), and a side it
//    closes cannot score thr.  Both bits travel with the work-list entry and the exact score walks
//    the arcs of the open side only (one v_min3 chain, fast_score_side); a wave that holds a pixel
//    with both sides open takes the two-sided form (fast_score_bytes) for all its lanes.  The bench
//    stream has no such pixel (profiles/fast_onesided_r07.md);
//  * non-max suppression runs over that survivor list, not over the tile: a list entry is the pixel's
//    byte index in the LDS score tile, its eight neighbours are eight byte reads;
//  * the 7x7 smoothing is two banded int8 GEMMs on the matrix cores (blur_tile_mfma).  In the
//    detection launch it runs last, on three waves, while the fourth waits for the atomic that
//    reserves the tile's slots in the candidate list;
//  * the integer min/max/SDWA ops issue at ~0.57x the fp32 rate on gfx950 (tools/ubench): the
//    kernel is VALU-issue bound, so the lever is instruction count, not bytes.
#include "frontend_common.h"
#include "../../include/vus_tiled.h"

namespace {

// ---- FAST tile kernels.  The -D knobs of this section: two occupancy knobs over the same code, two kinds of
// instrumentation build.  None of them selects between algorithms.
#ifndef VUS_FAST_WPE
#define VUS_FAST_WPE 1    // second __launch_bounds__ argument of the tile kernels: waves per SIMD the compiler must allow
#endif
#ifndef VUS_FAST_LDS_PAD
#define VUS_FAST_LDS_PAD 0   // occupancy experiment (tools/ab): dynamic LDS nobody uses = fewer workgroups per CU, same code
#endif
#ifdef VUS_FAST_EXIT_AFTER   // timing builds only (tools/ab): the tile kernel stops after phase N (1 .. 5), results are wrong
#define VUS_FAST_EXIT(N) do { if (VUS_FAST_EXIT_AFTER == (N)) return; } while (0)
#else
#define VUS_FAST_EXIT(N)
#endif
#ifdef VUS_FAST_DEBUG_COUNT   // counting build (tools/fast_counts.py): tiles, strips listed by pass 1a, pixels listed by pass 1b,
                              // wave-iterations of pass 2 and those of them that took the two-sided form (out: 5 values)
__device__ unsigned long long g_fast_dbg[5];
extern "C" int vus_debug_fast_counters(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fast_dbg), sizeof(g_fast_dbg)) != hipSuccess) return -1;
  if (reset) { unsigned long long z[5] = {0, 0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_fast_dbg), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#endif

// The tile shape is part of the ABI (the sampling pattern of vus_fast_threshold_estimate), and the kernel is written for
// it: the smoothing takes the 32 staged rows as its K, the late phases give the last of the four waves a job of its own.
constexpr int TW = VUS_FAST_TILE_W;     // output tile width  (1280 = 10 tiles of 128)
constexpr int TH = VUS_FAST_TILE_H;     // output tile height (720 = 30 tiles of 24)
constexpr int NTHREADS = 256;
// LDS images are arrays of dwords = 4 horizontally adjacent pixels ("strips"); the phases that walk the tile read
// ds_read_b32/b64 and unpack bytes in registers (byte-wide LDS reads cost ~3x the LDS cycles).
constexpr int IMG_ROWS = TH + 8;        // image rows  y0-4 .. y0+TH+3
constexpr int IMG_DW = (TW + 16) / 4;   // image cols  x0-8 .. x0+TW+7
constexpr int SC_ROWS = TH + 2;         // score rows  y0-1 .. y0+TH
constexpr int SC_DW = (TW + 8) / 4;     // score cols  x0-4 .. x0+TW+3
constexpr int STRIPS = TW / 4;          // strips of an output row

__device__ __forceinline__ int min3i(int a, int b, int c) { return min(min(a, b), c); }
__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }
__device__ __forceinline__ int byte_of(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xFFu); }

// FAST-9/16 score of a pixel from the sixteen circle bytes read as BYTES around it (c = its address in the staged tile,
// rb = bytes per staged row).  Sliding-window min / max of the 16 circle differences over every arc of 9:
//   w3[k] = op(d[k..k+2]),  w9[k] = op(w3[k], w3[k+3], w3[k+6]).
// Bright arcs need min(d) large, dark arcs need max(d) small (very negative).
// (Measured and not kept, round 4: the score from 7 x 3 dwords re-aligned with v_alignbyte so that the pixel sits at a
// fixed byte -- 21 ds_read_b32 + 21 v_alignbyte against the 17 ds_read_u8 here: 2.92 against 2.89 ms per 1000 stereo
// frames.  Round 3: the same windows on packed i16 pairs (b, 255 - b), one v_pk_min_i16 chain for bright and dark arcs --
// 95 packed instructions + 17 v_not do not issue faster than the ~160 scalar ones: fast_detect 6.23 against 6.17 ms.)
constexpr int FAST_DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
constexpr int FAST_DY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
__device__ __forceinline__ int fast_score_bytes(const uint8_t* c, int rb) {
  const int p = c[0];
  int d[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) d[k] = (int)c[FAST_DY[k] * rb + FAST_DX[k]] - p;
  int mn3[16], mx3[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    mn3[k] = min3i(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
    mx3[k] = max3i(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
  }
  int best_bright = -(1 << 20), best_dark = 1 << 20;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    best_bright = max(best_bright, min3i(mn3[k], mn3[(k + 3) & 15], mn3[(k + 6) & 15]));
    best_dark = min(best_dark, max3i(mx3[k], mx3[(k + 3) & 15], mx3[(k + 6) & 15]));
  }
  return max(best_bright, -best_dark) - 1;
}

// The same score for a pixel whose pre-test left ONE side open (flip = 0: the bright side, flip = 255: the dark side).
// Closed means that one of the tested opposite pairs has both members within thr of the pixel on that side; every arc
// of 9 holds a member of every opposite pair, so that side's best arc is worth at most thr - 1 and is never stored: the
// stored value is the open side's or nothing.  The windows are shift-invariant, so they run on the circle bytes
// themselves and the centre is subtracted once at the end; the dark side is the bright side of the complemented bytes
// (b ^ 255 = 255 - b), one full-rate v_xor per circle byte with the lane's flip where the two-sided form has a
// subtraction:  max over arcs of min(b ^ flip) - (p ^ flip) - 1  =  best_bright - 1  or  -best_dark - 1.
// 16 v_xor + 16 + 16 v_min3 + 8 v_max3 / v_max against 16 v_sub + 32 + 32 + 16 of the two-sided form.
// (The windows as the instruction itself: written as min(min(a, b), c) the compiler shares min(a, b) between
// neighbouring windows and ends with 38 v_min / v_min3 where 32 v_min3 do.)
__device__ __forceinline__ int min3_window(int a, int b, int c) {
  int r;
  asm("v_min3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int fast_score_side(const uint8_t* c, int rb, int flip) {
  int b[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) b[k] = (int)c[FAST_DY[k] * rb + FAST_DX[k]] ^ flip;
  int w3[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w3[k] = min3_window(b[k], b[(k + 1) & 15], b[(k + 2) & 15]);
  int w9[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w9[k] = min3_window(w3[k], w3[(k + 3) & 15], w3[(k + 6) & 15]);
  const int m0 = max3i(w9[0], w9[1], w9[2]), m1 = max3i(w9[3], w9[4], w9[5]), m2 = max3i(w9[6], w9[7], w9[8]);
  const int m3 = max3i(w9[9], w9[10], w9[11]), m4 = max3i(w9[12], w9[13], w9[14]);
  return max(max3i(m0, m1, m2), max3i(m3, m4, w9[15])) - ((int)c[0] ^ flip) - 1;
}

constexpr int VUS_CAND_REGIONS = 8;
// ---- the 7 x 7 smoothing of a staged tile on the matrix cores (round 4).  Both passes of the separable filter are
// products with a banded (Toeplitz) weight matrix, and v_mfma_i32_16x16x32_i8 computes a 16 x 16 block of such a
// product over a K window of 32 -- the 22 inputs a 16-wide block needs fit.  Exact integer arithmetic, same result as
// the definition (u16 row sums, then sum w H + 32768 >> 16):
//   H pass   C[row][col] = sum_k img[row][k] T[k][col]      A = 8 consecutive image bytes of a row (one ds_read_b64),
//            B = the weights, a per-lane constant.  The bytes are unsigned and the instruction is signed: a ^ 0x80 =
//            a - 128, and 128 * sum(w) = 32768 goes into the accumulator's initial value.
//   V pass   out^T[col][row] = sum_k H^T[col][k] Tv[k][row], with H split into its low and high bytes (two products,
//            recombined as (hi << 8) + lo).  K is only a summation index, so its order is chosen to be the one the
//            H pass leaves in the registers: lane (col, g) holds rows 4g..4g+3 of both 16-row blocks = its 8 K slots;
//            the weight operand is laid out to match.  No LDS round trip between the passes, and the result arrives as
//            4 consecutive pixels of one row per lane = one dword store.
// Cost per tile: 48 MFMAs and ~300 VALU wave-instructions against ~980 for the two-pass VALU form through
// LDS that it replaced (v_dot4_u32_u8 on v_alignbyte windows).
struct BlurMfmaTable {
  uint64_t h[64];      // H pass B operand: byte s of lane (g, n) = w[8 g + s - n - 5]
  uint64_t v[2][64];   // V pass B operand of output rows 16 nb + (lane & 15)
};
constexpr BlurMfmaTable make_blur_mfma_table() {
  constexpr int BW[7] = {18, 33, 49, 56, 49, 33, 18};
  BlurMfmaTable t{};
  for (int l = 0; l < 64; ++l) {
    const int g = l >> 4, m = l & 15;
    for (int sl = 0; sl < 8; ++sl) {
      const int d = 8 * g + sl - m - 5;     // image column 16 j + k feeds output column 16 j + n + 8 - 3 + tap
      if (d >= 0 && d <= 6) t.h[l] |= (uint64_t)BW[d] << (8 * sl);
      const int hrow = sl < 4 ? 4 * g + sl : 16 + 4 * g + (sl - 4);
      for (int nb = 0; nb < 2; ++nb) {
        const int dv = hrow - (16 * nb + m + 1);   // output row ly reads staged rows ly + 1 .. ly + 7
        if (dv >= 0 && dv <= 6) t.v[nb][l] |= (uint64_t)BW[dv] << (8 * sl);
      }
    }
  }
  return t;
}
__device__ __attribute__((aligned(16))) const BlurMfmaTable g_blur_mfma_table = make_blur_mfma_table();
typedef int v4i32_t __attribute__((ext_vector_type(4)));

// The tile's eight 16-column blocks go to the waves j_first, j_first + j_step, ... (all four waves: tid >> 6, 4; the
// late form below: three waves, the fourth waits for the tile's global atomic meanwhile).
// TILED: blur_out is block-tiled (include/vus_tiled.h; W % 16 == 0): a lane's 4 pixels lie in one 16-byte block row.
template <bool TILED = false>
__device__ __forceinline__ void blur_tile_mfma(const uint32_t* s_img, uint8_t* __restrict__ blur_out, int n, int H, int W,
                                               int x0, int y0, int tid, int j_first, int j_step) {
  static_assert(IMG_ROWS == 32 && TW % 16 == 0 && (IMG_DW * 4) % 8 == 0, "blur_tile_mfma: K = the 32 staged rows");
  const int l = tid & 63, g = l >> 4, m = l & 15;
  const long bh = (long)g_blur_mfma_table.h[l];
  const long bv[2] = {(long)g_blur_mfma_table.v[0][l], (long)g_blur_mfma_table.v[1][l]};
  const uint8_t* img8 = reinterpret_cast<const uint8_t*>(s_img);
  constexpr unsigned long long SIGN = 0x8080808080808080ull;
  // TILED: nothing about the bounds depends on the block.  Whole 16-column blocks (W % 16 == 0) make the x bound the
  // loop's uniform end, the y bounds are one lane mask per row block, and a lane's pixels of block j lie 128 j bytes
  // past those of block 0.
  const int j_end = TILED ? min(TW / 16, (W - x0) / 16) : TW / 16;
  bool row_ok[2] = {false, false};
  uint32_t tiled_off[2] = {0u, 0u};
  uint8_t* const tiled_plane = blur_out + (size_t)n * H * W;
  if (TILED) {
    j_first = __builtin_amdgcn_readfirstlane(j_first);   // a wave's blocks: the loop counter is a scalar
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int ly = 16 * nb + m;
      row_ok[nb] = ly < TH && y0 + ly < H;
      tiled_off[nb] = vus_tiled_offset(y0 + ly, x0 + 4 * g, W);
    }
  }
#pragma unroll 1   // (measured, round 4: other unroll factors change nothing)
  for (int j = j_first; j < j_end; j += j_step) {
    v4i32_t ch[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const unsigned long long a =
          *reinterpret_cast<const unsigned long long*>(img8 + (16 * mb + m) * (IMG_DW * 4) + 16 * j + 8 * g) ^ SIGN;
      const v4i32_t c0 = {32768, 32768, 32768, 32768};
      ch[mb] = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)a, bh, c0, 0, 0, 0);
    }
    // the 8 row sums of this lane (0 .. 65280) -> their low bytes and their high bytes, in K-slot order
    uint32_t lo[2], hi[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const uint32_t t0 = __builtin_amdgcn_perm((uint32_t)ch[mb][1], (uint32_t)ch[mb][0], 0x05010400u);
      const uint32_t t1 = __builtin_amdgcn_perm((uint32_t)ch[mb][3], (uint32_t)ch[mb][2], 0x05010400u);
      lo[mb] = __builtin_amdgcn_perm(t1, t0, 0x05040100u);
      hi[mb] = __builtin_amdgcn_perm(t1, t0, 0x07060302u);
    }
    const long a_lo = (long)((((unsigned long long)lo[1] << 32) | lo[0]) ^ SIGN);
    const long a_hi = (long)((((unsigned long long)hi[1] << 32) | hi[0]) ^ SIGN);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const v4i32_t ci = {32768, 32768, 32768, 32768};          // 128 * sum(w)
      const v4i32_t cl = {65536, 65536, 65536, 65536};          // 128 * sum(w) + the rounding half
      const v4i32_t chi = __builtin_amdgcn_mfma_i32_16x16x32_i8(a_hi, bv[nb], ci, 0, 0, 0);
      const v4i32_t clo = __builtin_amdgcn_mfma_i32_16x16x32_i8(a_lo, bv[nb], cl, 0, 0, 0);
      uint32_t q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = ((uint32_t)chi[r] << 8) + (uint32_t)clo[r];   // < 2^24: the pixel is byte 2
      const uint32_t v = __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0602u) | __builtin_amdgcn_perm(q[3], q[2], 0x06020c0cu);
      const int ly = 16 * nb + m, gy = y0 + ly, gx = x0 + 16 * j + 4 * g;
      if (TILED) {
        if (row_ok[nb]) __builtin_memcpy(tiled_plane + (tiled_off[nb] + (uint32_t)(VUS_TILE_BW * VUS_TILE_BH * j)), &v, 4);
      } else if (ly < TH && gy < H) {
        uint8_t* o = blur_out + ((size_t)n * H + gy) * W + gx;
        if (gx + 3 < W) {
          __builtin_memcpy(o, &v, 4);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gx + e < W) o[e] = (uint8_t)(v >> (8 * e));
        }
      }
    }
  }
}

// One 128 x 24 tile of image n, in phases:
//   staging     the 144 x 32 window into s_img, and the (min, max) of every staged dword into s_mm;
//   pass 1a     strip pre-test from the extrema: strips that may hold a corner are listed in s_strip (three passes of
//               the workgroup over the tile's own 32 x 24 strips, one short pass of two waves over the ring of 116);
//   pass 1b     per-pixel pre-test of the listed strips: pixels that may be corners are listed in s_work;
//   pass 2      exact score of the listed pixels into s_score (zeroed by pass 1a);
//   then, as the instance asks: the score tile written out (WRITE_SCORE); non-max suppression over s_work, the
//   survivors listed as keys and copied to the image's candidate list (DETECT) or counted by score into
//   hist[256 n + score] (DETECT + HIST: vus_fast_threshold_estimate's sample); the smoothing (BLUR).
// TILED (the late-smoothing detection launch only): blur_out is block-tiled (include/vus_tiled.h) and the tile's image
// goes to raw_out, block-tiled as well -- from the staged tile, by the wave that waits for the candidate atomic.
template <bool WRITE_SCORE, bool DETECT, bool BLUR, bool HIST = false, bool REGIONS = false, bool TILED = false>
__device__ __forceinline__ void fast_tile_body(
    const uint8_t* __restrict__ img, int H, int W, int pitch, int thr, int border,
    uint8_t* __restrict__ score_out, uint8_t* __restrict__ blur_out,
    uint32_t* __restrict__ cand_keys, int cand_cap, int* __restrict__ cand_count, int* __restrict__ hist,
    int n, int tile, int tiles_x, uint8_t* __restrict__ raw_out = nullptr) {
  static_assert(IMG_ROWS == 32, "the smoothing (blur_tile_mfma) takes the 32 staged rows as its K");
  constexpr bool SCORES = WRITE_SCORE || DETECT;   // the pre-tests and the exact score run; the blur-only instance skips them
  // LATE_BLUR (the detection launch proper): the smoothing runs at the END of the tile, on three waves, while the fourth
  // waits for the returning atomic that reserves the tile's slots in the image's candidate list.  The staged image then
  // has to live to the end: the candidate list moves to the strip tables' buffer (dead after pass 1b).  Otherwise the
  // smoothing runs after pass 1b on all four waves, and the list reuses the image tile, dead after the exact scores.
  constexpr bool LATE_BLUR = BLUR && DETECT && !HIST;
  static_assert(!TILED || LATE_BLUR, "the block-tiled planes are written by the late-smoothing detection launch");

  __shared__ __attribute__((aligned(8))) uint32_t s_img[IMG_ROWS * IMG_DW];
  __shared__ uint32_t s_score[SCORES ? SC_ROWS * SC_DW : 1];
  constexpr int AUX_DW = SCORES ? (IMG_ROWS * IMG_DW + SC_ROWS * SC_DW + 1) / 2 : 2;
  __shared__ uint32_t s_aux[AUX_DW];                               // the strip pre-test's two u16 tables:
  uint16_t* const s_mm = reinterpret_cast<uint16_t*>(s_aux);       // min | max << 8 of each staged dword
  uint16_t* const s_strip = s_mm + IMG_ROWS * IMG_DW;              // strips that pass the strip test
  // pixels that pass the pre-test: the pixel's byte index in the score tile (twelve bits) and, in the two top bits,
  // which sides of the pre-test it passed (WORK_BRIGHT, WORK_DARK)
  __shared__ uint16_t s_work[SCORES ? SC_ROWS * SC_DW * 4 : 2];
  constexpr int WORK_SIDE_SHIFT = 14, WORK_INDEX = (1 << 12) - 1;
  constexpr int WORK_BRIGHT = 1 << WORK_SIDE_SHIFT, WORK_DARK = 2 << WORK_SIDE_SHIFT;
  static_assert(SC_ROWS * SC_DW * 4 <= WORK_INDEX + 1, "a work-list entry keeps twelve bits for the pixel");
  __shared__ int s_nstrip;
  __shared__ int s_cnt, s_base, s_nwork;
  static_assert(IMG_ROWS * IMG_DW >= TW * TH / 4, "candidate list must fit in the image tile");
  static_assert(!LATE_BLUR || AUX_DW >= TW * TH / 4, "candidate list must fit in the strip tables' buffer");
  uint32_t* const s_keys = LATE_BLUR ? s_aux : s_img;

  const int tid = threadIdx.x;
  const int x0 = (tile % tiles_x) * TW, y0 = (tile / tiles_x) * TH;
  const uint8_t* im = img + (size_t)n * H * pitch;

  // stage the tile as dwords; out-of-image pixels replicate the border (what the smoothing wants;
  // FAST never produces a score within 3 pixels of the edge, so it does not care).
  // Thread = fixed dword column, 7 rows per pass: no per-element division, one address increment.
  {
    constexpr int RPP = NTHREADS / IMG_DW;   // rows per pass
    const int col = tid % IMG_DW, r0 = tid / IMG_DW;
    const int gx = x0 - 8 + 4 * col;
    const bool fast = gx >= 0 && gx + 3 < W;   // one dword load, aligned or not (odd-width pyramid levels)
    // tiles whose staged window lies inside the image (all but the frame of edge tiles) need no clamping: one
    // 32-bit offset per thread and a uniform row stride
    const bool inside = x0 >= 8 && x0 + TW + 8 <= W && y0 >= 4 && y0 + TH + 4 <= H;
    if (r0 < RPP) {
      // all loads of the thread are issued before the first is used (round 4: the per-row "load, wait, write" chain was
      // five global-memory latencies long); rows past the tile load a valid row again and are not written
      constexpr int NP = (IMG_ROWS + RPP - 1) / RPP;
      constexpr int LASTP = IMG_ROWS - (NP - 1) * RPP;   // threads with r0 < LASTP have a row in the last pass
      uint32_t v[NP];
      if (inside) {
        const uint32_t off0 = (uint32_t)((y0 - 4 + r0) * pitch + gx);
        const uint32_t step = (uint32_t)(RPP * pitch);
#pragma unroll
        for (int k = 0; k < NP - 1; ++k) __builtin_memcpy(&v[k], im + (off0 + (uint32_t)k * step), 4);
        v[NP - 1] = 0u;
        if (r0 < LASTP) __builtin_memcpy(&v[NP - 1], im + (off0 + (uint32_t)(NP - 1) * step), 4);
      } else {
        const uint8_t* rp[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) rp[k] = im + (size_t)clampi(y0 - 4 + min(r0 + RPP * k, IMG_ROWS - 1), 0, H - 1) * pitch;
        if (fast) {
#pragma unroll
          for (int k = 0; k < NP; ++k) __builtin_memcpy(&v[k], rp[k] + gx, 4);
        } else {
          const int c0 = clampi(gx, 0, W - 1), c1 = clampi(gx + 1, 0, W - 1), c2 = clampi(gx + 2, 0, W - 1),
                    c3 = clampi(gx + 3, 0, W - 1);
          uint8_t q[NP][4];
#pragma unroll
          for (int k = 0; k < NP; ++k) { q[k][0] = rp[k][c0]; q[k][1] = rp[k][c1]; q[k][2] = rp[k][c2]; q[k][3] = rp[k][c3]; }
#pragma unroll
          for (int k = 0; k < NP; ++k)
            v[k] = (uint32_t)q[k][0] | ((uint32_t)q[k][1] << 8) | ((uint32_t)q[k][2] << 16) | ((uint32_t)q[k][3] << 24);
        }
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int row = r0 + RPP * k;
        if (row < IMG_ROWS) {
          s_img[row * IMG_DW + col] = v[k];
          if (SCORES) {
            const int b0 = byte_of(v[k], 0), b1 = byte_of(v[k], 1), b2 = byte_of(v[k], 2), b3 = byte_of(v[k], 3);
            s_mm[row * IMG_DW + col] = (uint16_t)(min(min(b0, b1), min(b2, b3)) | (max(max(b0, b1), max(b2, b3)) << 8));
          }
        }
      }
    }
  }
  if (tid == 0) { s_cnt = 0; s_nwork = 0; s_nstrip = 0; }
  __syncthreads();
  VUS_FAST_EXIT(1);   // staging (+ per-dword extrema)

  if (SCORES) {
    // Pass 1 -- cheap necessary test on the pixels of the tile plus a ring (the 3x3 non-max suppression needs 1 pixel),
    // one strip of 4 per item.  A 9-long arc of the 16-circle always contains one pixel of every opposite pair, so a
    // corner needs  min over the tested pairs of max(pair) > p + thr  or  max over the pairs of min(pair) < p - thr
    // (pairs tested: N/S, E/W and the two diagonals).  Survivors are compacted into an LDS work list (wave prefix sum
    // with DPP, one LDS atomic per wave) so that pass 2 runs the full score on dense lanes.
    //
    // Pass 1a (round 4) -- an even cheaper necessary test per STRIP, from the per-dword extrema recorded while staging:
    // a pixel of the strip can pass the N/S + E/W pair test only if
    //    max(max N dword, max S dword) > min(strip) + thr  and  max(max W dword, max E dword, b0, b3) > min(strip) + thr
    // (its N/S neighbours are bytes of the dwords above / below, its W/E neighbours lie in the dword to the left plus
    // the strip's first byte / the strip's last byte plus the dword to the right), or the mirrored condition on the
    // dark side.  Measured on the configs[1] frames: 9.0 % of the strips pass at the adaptive threshold where 8.2 % hold
    // a pixel that passes the per-pixel test, 47 % against 45 % at fast_threshold 10 (single frames on the CPU; the
    // counting build on the bench stream says 18.2 % of a tile's strips are listed and 3.9 % of its pixels pass pass 1b).
    // The per-pixel test then runs on the listed strips only.
    // Thread = one strip of the tile proper: 32 x 24 strips = three full passes of the workgroup, eight rows of 32 per
    // pass (the LDS addresses of a pass differ from the first one's by constants).  The 116 strips of the ring (score
    // rows 0 and 25, score columns 0 and 33) take one further pass on waves 0 and 1, behind a wave-uniform branch.
    // All passes are evaluated first and listed with ONE LDS atomic per wave.
    static_assert(STRIPS == 32 && (TH * STRIPS) % NTHREADS == 0, "pass 1a: thread = (row tid >> 5, strip tid & 31)");
    constexpr int S_RPP = NTHREADS / STRIPS;                      // 8 rows of 32 strips per pass
    constexpr int NMAIN = TH / S_RPP;
    constexpr int NIT = NMAIN + 1;                                // + the ring pass
    static_assert(SC_DW + TH <= 64 && SC_ROWS == TH + 2 && SC_DW == STRIPS + 2, "pass 1a: the ring pass is a row and a column per wave");
    // the strip test proper; (sr, ss) = score row / strip column, ci = the strip's left neighbour in s_img / s_mm
    auto strip_test = [&](int sr, int ss, int ci) -> bool {
      const int gy = y0 - 1 + sr, gx = x0 - 4 + 4 * ss;
      // 0 <= gx < W - 3 and 3 <= gy < H - 3, one unsigned comparison each
      if (!((uint32_t)gx < (uint32_t)max(W - 3, 0) && (uint32_t)(gy - 3) < (uint32_t)max(H - 6, 0))) return false;
      // the (min, max) pairs read as the two bytes they are: ten ds_read_u8 instead of five ds_read_u16 + shifts /
      // masks (3.01 -> 2.96 ms per 1000 stereo frames)
      const uint8_t* mm8 = reinterpret_cast<const uint8_t*>(s_mm) + 2 * ci;
      const int ma_lo = mm8[0], ma_hi = mm8[1], pmin = mm8[2], pmax = mm8[3], mc_lo = mm8[4], mc_hi = mm8[5];
      const int mn_lo = mm8[2 - 6 * IMG_DW], mn_hi = mm8[3 - 6 * IMG_DW], ms_lo = mm8[2 + 6 * IMG_DW], ms_hi = mm8[3 + 6 * IMG_DW];
      const uint32_t b = s_img[ci + 1];
      const int b0 = byte_of(b, 0), b3 = byte_of(b, 3);
      const int hi = min(max(mn_hi, ms_hi), max3i(ma_hi, mc_hi, max(b0, b3)));
      const int lo = max(min(mn_lo, ms_lo), min3i(ma_lo, mc_lo, min(b0, b3)));
      return hi > pmin + thr || lo < pmax - thr;
    };
    const int sr0 = 1 + (tid >> 5), ss0 = 1 + (tid & 31);
    unsigned long long bal[NIT];
    bool pass[NIT];
    int ent[NIT];                                                 // s_strip entries
#pragma unroll
    for (int it = 0; it < NMAIN; ++it) {
      const int sr = sr0 + it * S_RPP;
      pass[it] = strip_test(sr, ss0, (sr0 + 3) * IMG_DW + ss0 + it * S_RPP * IMG_DW);
      s_score[sr0 * SC_DW + ss0 + it * S_RPP * SC_DW] = 0u;
      ent[it] = sr * SC_DW + ss0;
      bal[it] = __ballot(pass[it]);
    }
    pass[NMAIN] = false;
    ent[NMAIN] = 0;
    bal[NMAIN] = 0ull;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wv < 2) {
      // wave 0: score row 0, then column 0 of the rows between; wave 1: score row SC_ROWS - 1, then column SC_DW - 1
      const int l = tid & 63;
      const bool is_row = l < SC_DW;
      const int sr = is_row ? wv * (SC_ROWS - 1) : l - (SC_DW - 1);
      const int ss = is_row ? l : wv * (SC_DW - 1);
      if (l < SC_DW + TH) {
        pass[NMAIN] = strip_test(sr, ss, (sr + 3) * IMG_DW + ss);
        s_score[sr * SC_DW + ss] = 0u;
        ent[NMAIN] = sr * SC_DW + ss;
      }
      bal[NMAIN] = __ballot(pass[NMAIN]);
    }
    int total = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) total += __popcll(bal[it]);
    if (total > 0) {
      int base = 0;
      if ((tid & 63) == 0) base = atomicAdd(&s_nstrip, total);
      base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        if (pass[it])
          s_strip[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[it] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[it], 0))] =
              (uint16_t)ent[it];
        base += __popcll(bal[it]);
      }
    }
    __syncthreads();
    VUS_FAST_EXIT(2);   // + strip pre-test
    const int nstrip = s_nstrip;
#ifdef VUS_FAST_DEBUG_COUNT
    if (tid == 0 && BLUR) { atomicAdd(&g_fast_dbg[0], 1ull); atomicAdd(&g_fast_dbg[1], (unsigned long long)nstrip); }
#endif
    // Pass 1b -- the per-pixel test, one listed strip per lane.
    // (Measured and not kept, round 4: the same test with one PIXEL per lane -- nine byte reads, no v_alignbyte / v_bfe,
    // work spread over all four waves: bit-exact, 3.00 against 2.92 ms per 1000 stereo frames.  A tile lists 161 of its
    // 884 strips here and 138 of their pixels go on to the exact score, tools/fast_counts.py.)
    for (int j0 = 0; j0 < nstrip; j0 += NTHREADS) {   // uniform trip count (wave scans inside)
      const int j = j0 + tid;
      // side[e]: the pre-test's two comparisons for pixel e of the strip as its two low bits -- bit 0: the bright side is
      // open, bit 1: the dark side -- above them those of the pixels before it.  Each comparison is the sign of a
      // difference, shifted in with one v_alignbit: side[3] holds all eight.
      uint32_t side[4] = {0u, 0u, 0u, 0u};
      int idx = 0;
      if (j < nstrip) {
        idx = s_strip[j];
        const int sr = idx / SC_DW, ss = idx - sr * SC_DW;
        const int gx = x0 - 4 + 4 * ss;
        const uint32_t* cp = &s_img[(sr + 3) * IMG_DW + ss];
        const uint32_t a = cp[0], b = cp[1], c = cp[2];
        const uint32_t nn = s_img[sr * IMG_DW + ss + 1], so = s_img[(sr + 6) * IMG_DW + ss + 1];
        const uint32_t wv = __builtin_amdgcn_alignbyte(b, a, 1);   // bytes x-3 of the 4 pixels
        const uint32_t ev = __builtin_amdgcn_alignbyte(c, b, 3);   // bytes x+3
        // the diagonal opposite pairs of the circle, (x+2,y-2)/(x-2,y+2) and (x+2,y+2)/(x-2,y-2): with them 25 % of the
        // pixels pass the pre-test instead of 33 %, fast_detect 6.32 -> 6.23 ms.  (Measured and not kept: all eight
        // opposite pairs -- 22.7 % pass, the four more pairs cost more than the fewer exact scores save.)
        const uint32_t* up = &s_img[(sr + 1) * IMG_DW + ss];
        const uint32_t* dn = &s_img[(sr + 5) * IMG_DW + ss];
        const uint32_t nev = __builtin_amdgcn_alignbyte(up[2], up[1], 2), nwv = __builtin_amdgcn_alignbyte(up[1], up[0], 2);
        const uint32_t sev = __builtin_amdgcn_alignbyte(dn[2], dn[1], 2), swv = __builtin_amdgcn_alignbyte(dn[1], dn[0], 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int p = byte_of(b, e);
          const int n_ = byte_of(nn, e), s_ = byte_of(so, e), w_ = byte_of(wv, e), e_ = byte_of(ev, e);
          int hi = min(max(n_, s_), max(e_, w_)), lo = max(min(n_, s_), min(e_, w_));
          const int ne = byte_of(nev, e), sw = byte_of(swv, e), se = byte_of(sev, e), nw = byte_of(nwv, e);
          hi = min3i(hi, max(ne, sw), max(se, nw));
          lo = max3i(lo, min(ne, sw), min(se, nw));
          // hi > p + thr: the bright side is open; lo < p - thr: the dark side
          const uint32_t dark = __builtin_amdgcn_alignbit(e ? side[e - 1] : 0u, (uint32_t)(lo - (p - thr)), 31);
          side[e] = __builtin_amdgcn_alignbit(dark, (uint32_t)((p + thr) - hi), 31);
        }
        if (gx < 3 || gx + 3 >= W - 3) {   // strips straddling the 3-pixel frame (edge tiles only)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gx + e < 3 || gx + e >= W - 3) {
              side[e] &= ~3u;
              side[3] &= ~(3u << (2 * (3 - e)));
            }
        }
      }
      const uint32_t listed = (side[3] | (side[3] >> 1)) & 0x55u;   // bit 2 (3 - e): pixel e goes on to the exact score
      const int cnt = __popc(listed);
      int incl = cnt;   // inclusive wave scan (same DPP sequence as wave_sum_i32)
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xe, true);
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xc, true);
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, true);
      incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, true);
      const int total = __builtin_amdgcn_readlane(incl, 63);
      int base = 0;
      if ((tid & 63) == 0 && total > 0) base = atomicAdd(&s_nwork, total);
      base = __builtin_amdgcn_readfirstlane(base);
      int pos = base + incl - cnt;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (listed & (1u << (2 * (3 - e)))) s_work[pos++] = (uint16_t)(side[e] << WORK_SIDE_SHIFT | (uint32_t)(idx * 4 + e));   // the store keeps 16 bits
    }
  }
#ifdef VUS_FAST_DEBUG_COUNT
  __syncthreads();
  if (tid == 0 && BLUR && SCORES) atomicAdd(&g_fast_dbg[2], (unsigned long long)s_nwork);
#endif
  VUS_FAST_EXIT(3);   // + per-pixel pre-test of the listed strips
  if (BLUR && !LATE_BLUR) blur_tile_mfma(s_img, blur_out, n, H, W, x0, y0, tid, tid >> 6, NTHREADS / 64);   // reads the staged tile only: no barrier of its own
  __syncthreads();
  VUS_FAST_EXIT(4);   // + smoothing

  if (SCORES) {
    // Pass 2 -- exact FAST score of the survivors, one pixel per lane, from the bytes around it in the staged tile.
    // A pixel that passed one side of the pre-test walks that side's arcs only (fast_score_side): the other side cannot
    // reach thr.  A pixel that passed both (a mid-grey pixel on an edge of contrast above 2 thr that runs between the
    // tested pairs; none on the bench stream) needs both chains: a wave with such a lane takes the two-sided form for
    // all its lanes, behind one ballot.
    const int nwork = s_nwork;
    uint8_t* score8 = reinterpret_cast<uint8_t*>(s_score);
    for (int j = tid; j < nwork; j += NTHREADS) {
      const int went = s_work[j];
      const int ent = went & WORK_INDEX;
      const int idx = ent >> 2, e = ent & 3;
      const int sr = idx / SC_DW, ss = idx - sr * SC_DW;
      const uint8_t* c = reinterpret_cast<const uint8_t*>(s_img) + (sr + 3) * (4 * IMG_DW) + 4 * (ss + 1) + e;
      int sc;
      const bool two_sided = __ballot((went & (WORK_BRIGHT | WORK_DARK)) == (WORK_BRIGHT | WORK_DARK)) != 0ull;
#ifdef VUS_FAST_DEBUG_COUNT
      if (j == __builtin_amdgcn_readfirstlane(j) && BLUR) { atomicAdd(&g_fast_dbg[3], 1ull); atomicAdd(&g_fast_dbg[4], two_sided ? 1ull : 0ull); }
#endif
      if (two_sided) {
        sc = fast_score_bytes(c, 4 * IMG_DW);
      } else {
        sc = fast_score_side(c, 4 * IMG_DW, (went & WORK_BRIGHT) ? 0 : 255);
      }
      if (sc >= thr) score8[ent] = (uint8_t)sc;
    }
    __syncthreads();
  }
  VUS_FAST_EXIT(5);   // + exact scores

  if (WRITE_SCORE) {
    for (int idx = tid; idx < TH * STRIPS; idx += NTHREADS) {
      const int ly = idx / STRIPS, ls = idx - ly * STRIPS;
      const int gy = y0 + ly, gx = x0 + 4 * ls;
      const uint32_t v = s_score[(ly + 1) * SC_DW + ls + 1];
      if (gy < H) {
        uint8_t* o = score_out + ((size_t)n * H + gy) * W + gx;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gx + e < W) o[e] = (uint8_t)(v >> (8 * e));
      }
    }
  }
  if (DETECT) {
    // Non-max suppression over the SURVIVOR LIST of pass 2, not over the tile (round 4): with the adaptive threshold a
    // tile keeps a few hundred scored pixels of 3536, yet nearly every 4-pixel strip of a wave's 64 had one in it, so the
    // strip loop ran its 3 x 3-dword windows for the whole tile (~700 of the tile's ~4600 wave-instructions).  A list
    // entry is the pixel's byte index in the score tile: its eight neighbours are eight byte reads.
    const int nwork = s_nwork;
    const uint8_t* score8 = reinterpret_cast<const uint8_t*>(s_score);
    for (int j = tid; j < nwork; j += NTHREADS) {
      const int ent = s_work[j] & WORK_INDEX;
      const int s = score8[ent];
      if (s == 0) continue;
      const int sr = ent / (4 * SC_DW), sx = ent - sr * (4 * SC_DW);     // row / byte column inside the score tile
      const int ly = sr - 1, lx = sx - 4;                                 // the ring belongs to the neighbouring tiles
      if (ly < 0 || ly >= TH || lx < 0 || lx >= TW) continue;
      const int gy = y0 + ly, gx = x0 + lx;
      if (gy < border || gy >= H - border || gx < border || gx >= W - border) continue;
      const uint8_t* c = score8 + ent;
      constexpr int RB = 4 * SC_DW;
      // (int operands throughout: max() of two bytes against an int resolved to the double overload -- six fp64
      // conversions and maxima per survivor)
      const int m = max3i(max3i(c[-RB - 1], c[-RB], c[-RB + 1]), max((int)c[-1], (int)c[1]), max3i(c[RB - 1], c[RB], c[RB + 1]));
      if (s > m) {                                                         // strict maximum of its 8 neighbours
        if (HIST) {
          atomicAdd(&hist[256 * n + s], 1);       // a sampled tile yields a few dozen survivors: no LDS stage
        } else {
          const int p = atomicAdd(&s_cnt, 1);
          s_keys[p] = ((uint32_t)(255 - s) << VUS_KEY_POS_BITS) | (uint32_t)(gy * W + gx);
        }
      }
    }
    if (!HIST) {
      __syncthreads();
      const int cnt = s_cnt;
      // REGIONS: the image's list is filled as VUS_CAND_REGIONS sub-lists, tile t into region t mod 8, each with its counter in
      // its own first slot (cand_region_merge_kernel compacts them afterwards): the ~300 returning atomics of an image on
      // ONE word serialised at the memory side -- 0.14 of the launch's 2.93 ms (timing build with eight counters on lines
      // of their own)
      const int rcap = cand_cap / VUS_CAND_REGIONS;
      uint32_t* const list = cand_keys + (size_t)n * cand_cap + (REGIONS ? (size_t)(tile & (VUS_CAND_REGIONS - 1)) * rcap : 0);
      int* const counter = REGIONS ? reinterpret_cast<int*>(list) : &cand_count[n];
      if (LATE_BLUR) {
        const bool leader = tid == NTHREADS - 64 && cnt > 0;
        int base = 0;
        if (leader) base = atomicAdd(counter, cnt);
        if (TILED && tid >= NTHREADS - 64) {
          // the staged tile's interior, block-tiled: TH x TW / 16 rows of 16 bytes (whole blocks: x0 % 16 == 0,
          // y0 % 8 == 0, W % 16 == 0, H % 8 == 0), three per lane, while the atomic is out
          const uint8_t* s8 = reinterpret_cast<const uint8_t*>(s_img);
          uint8_t* const ro = raw_out + (size_t)n * H * W;
          for (int i = tid - (NTHREADS - 64); i < TH * (TW / 16); i += 64) {
            const int ly = i / (TW / 16), cb = i - ly * (TW / 16);
            const int gy = y0 + ly, gx = x0 + 16 * cb;
            if (gy < H && gx < W) {
              const uint8_t* sp = s8 + (ly + 4) * (4 * IMG_DW) + 8 + 16 * cb;   // 8-byte aligned
              const uint2 a = *reinterpret_cast<const uint2*>(sp), b = *reinterpret_cast<const uint2*>(sp + 8);
              *reinterpret_cast<uint4*>(ro + vus_tiled_offset(gy, gx, W)) = make_uint4(a.x, a.y, b.x, b.y);
            }
          }
        }
        if (leader) s_base = base;
        if (tid < NTHREADS - 64) blur_tile_mfma<TILED>(s_img, blur_out, n, H, W, x0, y0, tid, tid >> 6, NTHREADS / 64 - 1);
      } else {
        if (tid == 0 && cnt > 0) s_base = atomicAdd(counter, cnt);
      }
      __syncthreads();
      if (cnt > 0) {
        const int base = s_base + (REGIONS ? 1 : 0), lim = REGIONS ? rcap : cand_cap;
        for (int i = tid; i < cnt; i += NTHREADS)
          if (base + i < lim) list[base + i] = s_keys[i];
      }
    }
  }
}

// XCD-aware block -> (image, tile) map: blocks with equal (blockIdx % 8) share an XCD, so all tiles of one
// image run on ONE XCD and the halo re-reads of neighbouring tiles hit its L2 instead of HBM (speed only).
// thr_img (may be null): per-image thresholds of the adaptive detector (vus_fast_detect_adaptive).
template <bool WRITE_SCORE, bool DETECT, bool BLUR, bool REGIONS = false>
__global__ __launch_bounds__(NTHREADS, VUS_FAST_WPE) void fast_tile_kernel(
    const uint8_t* __restrict__ img, int H, int W, int pitch, int thr, const int* __restrict__ thr_img, int border,
    uint8_t* __restrict__ score_out, uint8_t* __restrict__ blur_out,
    uint32_t* __restrict__ cand_keys, int cand_cap, int* __restrict__ cand_count, int n_img, int tiles_x,
    int tiles_per_img) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int n = (slot / tiles_per_img) * 8 + xcd;
  if (n >= n_img) return;
  const int tile = slot - (slot / tiles_per_img) * tiles_per_img;
  fast_tile_body<WRITE_SCORE, DETECT, BLUR, false, REGIONS>(img, H, W, pitch, thr_img ? thr_img[n] : thr, border, score_out, blur_out,
                                                            cand_keys, cand_cap, cand_count, nullptr, n, tile, tiles_x);
}

// fast_tile_kernel<false, true, true, REGIONS> with both planes block-tiled (vus_fast_detect_adaptive_tiled)
template <bool REGIONS>
__global__ __launch_bounds__(NTHREADS, VUS_FAST_WPE) void fast_tile_tiled_kernel(
    const uint8_t* __restrict__ img, int H, int W, int pitch, const int* __restrict__ thr_img, int border,
    uint8_t* __restrict__ blur_out, uint8_t* __restrict__ raw_out, uint32_t* __restrict__ cand_keys, int cand_cap,
    int* __restrict__ cand_count, int n_img, int tiles_x, int tiles_per_img) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int n = (slot / tiles_per_img) * 8 + xcd;
  if (n >= n_img) return;
  const int tile = slot - (slot / tiles_per_img) * tiles_per_img;
  fast_tile_body<false, true, true, false, REGIONS, true>(img, H, W, pitch, thr_img[n], border, nullptr, blur_out, cand_keys,
                                                          cand_cap, cand_count, nullptr, n, tile, tiles_x, raw_out);
}

// The regions of fast_tile_kernel<.., REGIONS>: counters zeroed before the launch ...
__global__ void cand_region_zero_kernel(uint32_t* __restrict__ cand_keys, int cand_cap, int n_img) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_img * VUS_CAND_REGIONS)
    cand_keys[(size_t)(t / VUS_CAND_REGIONS) * cand_cap + (size_t)(t % VUS_CAND_REGIONS) * (cand_cap / VUS_CAND_REGIONS)] = 0u;
}

// ... and compacted after it, one workgroup per image: region r's keys (slots 1 .. of its part of the row) move down to
// where region r - 1's ended -- always to lower addresses than anything still unread, a chunk read whole before it is
// written -- and cand_count[n] becomes the total.  A region that overflowed its share of cand_cap is reported as an
// overflow of the list: cand_count[n] > cand_cap, the unwritten tail filled with VUS_KEY_INVALID.  That happens well below
// cand_cap whenever the candidates crowd into the tiles of one region: a textured patch inside a single 128-pixel tile
// column is such a layout whenever tiles_x is a multiple of 8 (widths 897 .. 1024), and nearly so for tiles_x = 2, 4, 6.
// vus_fast_detect_retry detects such an image again into a single list.
__global__ __launch_bounds__(256) void cand_region_merge_kernel(uint32_t* __restrict__ cand_keys, int cand_cap, int* __restrict__ cand_count) {
  __shared__ int s_c[VUS_CAND_REGIONS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int rcap = cand_cap / VUS_CAND_REGIONS;
  uint32_t* row = cand_keys + (size_t)n * cand_cap;
  if (tid < VUS_CAND_REGIONS) s_c[tid] = (int)row[(size_t)tid * rcap];
  __syncthreads();
  int off = 0;
  long long all = 0;
  bool over = false;
  for (int r = 0; r < VUS_CAND_REGIONS; ++r) {
    const int c = s_c[r], m = min(c, rcap - 1);
    all += c;
    over |= c > rcap - 1;
    const uint32_t* src = row + (size_t)r * rcap + 1;
    for (int i0 = 0; i0 < m; i0 += 256) {
      const int i = i0 + tid;
      const uint32_t v = i < m ? src[i] : 0u;
      __syncthreads();
      if (i < m) row[off + i] = v;
      __syncthreads();
    }
    off += m;
  }
  if (over)
    for (int i = off + tid; i < cand_cap; i += 256) row[i] = VUS_KEY_INVALID;
  if (tid == 0) cand_count[n] = over ? (int)max(all, (long long)cand_cap + 1) : off;
}

// ---- the adaptive detector (round 4): the top-K keypoints of an image depend only on pixels whose score reaches s*,
// the K-th best score among the non-max-suppression survivors.  A pixel below s* can neither be selected nor suppress a
// pixel at or above it (suppression needs a neighbour with a score >= its own).  So detection at ANY threshold
// t' <= s* gives the same top K as detection at fast_threshold -- and far fewer pixels pass the pre-test of pass 1 and
// reach the exact score of pass 2, where the kernel's instructions go (configs[1]: s* ~ 128, 25 % of the pixels pass the
// pre-test at 10, ~5 % at 110).  t' is estimated per image from the survivors' score histogram of a SAMPLE of tiles
// (every sample_stride-th tile, at fast_threshold), with a margin; whether the estimate was good enough is CHECKED on
// the device (did the image yield >= K candidates?), and the images that failed are detected again at fast_threshold.
// Bit-identical keypoints by construction, whatever the estimate.
__global__ __launch_bounds__(NTHREADS, VUS_FAST_WPE) void fast_sample_kernel(const uint8_t* __restrict__ img, int H, int W, int pitch,
                                                               int thr, int border, int* __restrict__ hist, int n_img,
                                                               int tiles_x, int tiles_per_img, int stride, int n_sampled) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int n = (slot / n_sampled) * 8 + xcd;
  if (n >= n_img) return;
  const int tile = (slot - (slot / n_sampled) * n_sampled) * stride + stride / 2;
  if (tile >= tiles_per_img) return;
  fast_tile_body<false, true, false, true>(img, H, W, pitch, thr, border, nullptr, nullptr, nullptr, 0, nullptr, hist, n, tile, tiles_x);
}

// thr_img[n] = the largest t in (floor, 254] with  (survivors of the sample with score >= t) * n_tiles * den  >=
// max_kp * n_sampled * num  (num / den: the margin), thr if there is none (floor = the threshold the sample was detected
// at, >= thr: the bins below it are empty).  One thread per image.
__global__ __launch_bounds__(256) void fast_pick_threshold_kernel(const int* __restrict__ hist, int n_img, int thr, int floor, int max_kp,
                                                                  long long n_tiles, long long n_sampled, int num, int den,
                                                                  int* __restrict__ thr_img) {
  // one WAVE per image (one thread per image walked its 200 bins as 200 dependent loads: 29 us for 2000 images): lane l
  // holds bins 4 l .. 4 l + 3, a suffix scan over the lanes gives every bin its count(score >= t), the largest
  // qualifying t wins
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= n_img) return;
  const int4 h = reinterpret_cast<const int4*>(hist + 256 * (size_t)n)[lane];
  const int hv[4] = {h.x, h.y, h.z, lane == 63 ? 0 : h.w};        // bin 255 is never counted (scores end at 254)
  int above = hv[0] + hv[1] + hv[2] + hv[3];                       // -> sum over the lanes ABOVE this one
  int incl = above;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_down(incl, d);
    if (lane + d < 64) incl += o;
  }
  above = incl - above;
  const long long need = (long long)max_kp * n_sampled * num;
  long long run = above;
  int best = -1;
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    run += hv[q];
    const int t = 4 * lane + q;
    if (best < 0 && t > floor && t <= 254 && run * n_tiles * den >= need) best = t;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
  if (lane == 0) thr_img[n] = best > floor ? best : thr;
}

// images whose adaptive pass yielded fewer than max_kp candidates although it ran above fast_threshold, and images whose
// list overflowed (a sub-list that outgrew its share is reported as one, cand_region_merge_kernel; a true overflow stays
// one, with its true count, after the single-list detection at fast_threshold): listed, their counts reset (one workgroup)
__global__ __launch_bounds__(1024) void fast_retry_list_kernel(const int* __restrict__ thr_img, int thr, int max_kp, int cand_cap,
                                                               int n_img, int* __restrict__ cand_count,
                                                               int* __restrict__ retry_list, int* __restrict__ retry_count) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  for (int n = threadIdx.x; n < n_img; n += 1024)
    if ((thr_img[n] > thr && cand_count[n] < max_kp) || cand_count[n] > cand_cap) {
      retry_list[atomicAdd(&s_n, 1)] = n;
      cand_count[n] = 0;
    }
  __syncthreads();
  if (threadIdx.x == 0) retry_count[0] = s_n;
}

// persistent: (listed image, tile) items at fast_threshold; no work, no cost.  The loop around the tile body keeps more
// alive than the one-tile kernels do: asked for seven waves per SIMD the compiler fits it into 72 VGPRs without scratch
// (78 and six waves if left alone).
__global__ __launch_bounds__(NTHREADS, VUS_FAST_WPE > 7 ? VUS_FAST_WPE : 7) void fast_retry_kernel(const uint8_t* __restrict__ img, int H, int W, int pitch, int thr,
                                                              int border, uint32_t* __restrict__ cand_keys, int cand_cap,
                                                              int* __restrict__ cand_count, const int* __restrict__ retry_list,
                                                              const int* __restrict__ retry_count, int tiles_x, int tiles_per_img) {
  const long long items = (long long)retry_count[0] * tiles_per_img;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = retry_list[it / tiles_per_img], tile = (int)(it % tiles_per_img);
    fast_tile_body<false, true, false>(img, H, W, pitch, thr, border, nullptr, nullptr, cand_keys, cand_cap, cand_count, nullptr, n,
                                       tile, tiles_x);
    __syncthreads();                 // the tile's LDS images are reused by the next item
  }
}

struct TileGrid {
  unsigned blocks;
  int tiles_x, tiles_per_img;
};
TileGrid tile_grid(int n_img, int H, int W) {
  const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;
  return TileGrid{(unsigned)(((n_img + 7) / 8) * 8 * tx * ty), tx, tx * ty};
}

}  // namespace

extern "C" int vus_fast_score(const uint8_t* img, int n_img, int H, int W, int pitch, int thr,
                              uint8_t* score_out, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(score_out != nullptr, "score_out is null");
  VUS_REQUIRE(thr >= 1 && thr <= 254, "thr=%d out of range [1, 254]", thr);
  if (n_img == 0) return VUS_OK;
  const TileGrid g = tile_grid(n_img, H, W);
  fast_tile_kernel<true, false, false><<<g.blocks, NTHREADS, 0, vus::as_stream(stream)>>>(
      img, H, W, pitch, thr, nullptr, 0, score_out, nullptr, nullptr, 0, nullptr, n_img, g.tiles_x, g.tiles_per_img);
  VUS_CHECK_LAUNCH("fast_score");
  return VUS_OK;
}

extern "C" int vus_blur7(const uint8_t* img, int n_img, int H, int W, int pitch, uint8_t* out, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(out != nullptr, "out is null");
  if (n_img == 0) return VUS_OK;
  const TileGrid g = tile_grid(n_img, H, W);
  fast_tile_kernel<false, false, true><<<g.blocks, NTHREADS, 0, vus::as_stream(stream)>>>(
      img, H, W, pitch, 1, nullptr, 0, nullptr, out, nullptr, 0, nullptr, n_img, g.tiles_x, g.tiles_per_img);
  VUS_CHECK_LAUNCH("blur7");
  return VUS_OK;
}

extern "C" int vus_fast_detect(const uint8_t* img, int n_img, int H, int W, int pitch, int thr, int border,
                               uint8_t* blur_out, uint32_t* cand_keys, int cand_cap, int* cand_count,
                               void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(cand_keys != nullptr && cand_count != nullptr, "candidate buffers are null");
  VUS_REQUIRE(cand_cap >= 1, "cand_cap=%d", cand_cap);
  VUS_REQUIRE(thr >= 1 && thr <= 254, "thr=%d out of range [1, 254]", thr);
  VUS_REQUIRE(border >= 0, "border=%d", border);
  if (n_img == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const TileGrid g = tile_grid(n_img, H, W);
  if (blur_out)
    fast_tile_kernel<false, true, true><<<g.blocks, NTHREADS, 0, st>>>(
        img, H, W, pitch, thr, nullptr, border, nullptr, blur_out, cand_keys, cand_cap, cand_count, n_img, g.tiles_x,
        g.tiles_per_img);
  else
    fast_tile_kernel<false, true, false><<<g.blocks, NTHREADS, 0, st>>>(
        img, H, W, pitch, thr, nullptr, border, nullptr, nullptr, cand_keys, cand_cap, cand_count, n_img, g.tiles_x,
        g.tiles_per_img);
  VUS_CHECK_LAUNCH("fast_detect");
  return VUS_OK;
}

extern "C" int vus_fast_threshold_estimate(const uint8_t* img, int n_img, int H, int W, int pitch, int thr, int border,
                                           int max_kp, int sample_stride, int* hist, int* thr_img, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(hist != nullptr && thr_img != nullptr, "null buffer");
  VUS_REQUIRE(thr >= 1 && thr <= 254, "thr=%d out of range [1, 254]", thr);
  VUS_REQUIRE(border >= 0 && max_kp >= 1 && sample_stride >= 1, "border=%d max_kp=%d sample_stride=%d", border, max_kp, sample_stride);
  if (n_img == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const TileGrid g = tile_grid(n_img, H, W);
  const int n_sampled = (g.tiles_per_img - sample_stride / 2 + sample_stride - 1) / sample_stride;     // tiles S/2, S/2 + S, ...
  VUS_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int) * 256 * (size_t)n_img, st));
  // the sample runs at max(thr, VUS_FAST_SAMPLE_FLOOR): an estimate is only ever taken from the bins above that, and at
  // thr = 10 half of a tile's strips pass the pre-tests (the sample cost 0.16 ms per 1000 stereo frames, a twentieth of the
  // detection it serves)
  const int floor = thr > VUS_FAST_SAMPLE_FLOOR ? thr : VUS_FAST_SAMPLE_FLOOR;
  if (n_sampled > 0)
    fast_sample_kernel<<<(unsigned)(((n_img + 7) / 8) * 8 * n_sampled), NTHREADS, 0, st>>>(
        img, H, W, pitch, floor, border, hist, n_img, g.tiles_x, g.tiles_per_img, sample_stride, n_sampled);
  fast_pick_threshold_kernel<<<(n_img + 3) / 4, 256, 0, st>>>(hist, n_img, thr, floor, max_kp, g.tiles_per_img,
                                                                 n_sampled > 0 ? n_sampled : 1, VUS_FAST_MARGIN_NUM,
                                                                 VUS_FAST_MARGIN_DEN, thr_img);
  VUS_CHECK_LAUNCH("fast_threshold_estimate");
  return VUS_OK;
}

extern "C" int vus_fast_detect_adaptive(const uint8_t* img, int n_img, int H, int W, int pitch, const int* thr_img, int border,
                                        uint8_t* blur_out, uint32_t* cand_keys, int cand_cap, int* cand_count, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(cand_keys != nullptr && cand_count != nullptr && thr_img != nullptr, "null buffer");
  VUS_REQUIRE(cand_cap >= 1 && border >= 0, "cand_cap=%d border=%d", cand_cap, border);
  if (n_img == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const TileGrid g = tile_grid(n_img, H, W);
  // with room for it, the list is filled as eight sub-lists and compacted afterwards (fast_tile_body, REGIONS)
  const bool regions = blur_out != nullptr && cand_cap >= 64 * VUS_CAND_REGIONS;
  if (regions) {
    cand_region_zero_kernel<<<(n_img * VUS_CAND_REGIONS + 255) / 256, 256, 0, st>>>(cand_keys, cand_cap, n_img);
    fast_tile_kernel<false, true, true, true><<<g.blocks, NTHREADS, VUS_FAST_LDS_PAD, st>>>(
        img, H, W, pitch, 0, thr_img, border, nullptr, blur_out, cand_keys, cand_cap, cand_count, n_img, g.tiles_x, g.tiles_per_img);
    cand_region_merge_kernel<<<n_img, 256, 0, st>>>(cand_keys, cand_cap, cand_count);
  } else if (blur_out)
    fast_tile_kernel<false, true, true><<<g.blocks, NTHREADS, VUS_FAST_LDS_PAD, st>>>(
        img, H, W, pitch, 0, thr_img, border, nullptr, blur_out, cand_keys, cand_cap, cand_count, n_img, g.tiles_x, g.tiles_per_img);
  else
    fast_tile_kernel<false, true, false><<<g.blocks, NTHREADS, 0, st>>>(
        img, H, W, pitch, 0, thr_img, border, nullptr, nullptr, cand_keys, cand_cap, cand_count, n_img, g.tiles_x, g.tiles_per_img);
  VUS_CHECK_LAUNCH("fast_detect_adaptive");
  return VUS_OK;
}

extern "C" int vus_fast_detect_adaptive_tiled(const uint8_t* img, int n_img, int H, int W, int pitch, const int* thr_img,
                                              int border, uint8_t* blur_tiled, uint8_t* img_tiled, uint32_t* cand_keys,
                                              int cand_cap, int* cand_count, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  if (int rc = check_tiled_args(blur_tiled, img_tiled, H, W)) return rc;
  VUS_REQUIRE(cand_keys != nullptr && cand_count != nullptr && thr_img != nullptr, "null buffer");
  VUS_REQUIRE(cand_cap >= 1 && border >= 0, "cand_cap=%d border=%d", cand_cap, border);
  if (n_img == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const TileGrid g = tile_grid(n_img, H, W);
  static_assert(TW % VUS_TILE_BW == 0 && TH % VUS_TILE_BH == 0, "a detector tile is whole blocks");
  // the same list scheme as vus_fast_detect_adaptive with a smoothing plane
  if (cand_cap >= 64 * VUS_CAND_REGIONS) {
    cand_region_zero_kernel<<<(n_img * VUS_CAND_REGIONS + 255) / 256, 256, 0, st>>>(cand_keys, cand_cap, n_img);
    fast_tile_tiled_kernel<true><<<g.blocks, NTHREADS, 0, st>>>(img, H, W, pitch, thr_img, border, blur_tiled, img_tiled,
                                                                cand_keys, cand_cap, cand_count, n_img, g.tiles_x, g.tiles_per_img);
    cand_region_merge_kernel<<<n_img, 256, 0, st>>>(cand_keys, cand_cap, cand_count);
  } else {
    fast_tile_tiled_kernel<false><<<g.blocks, NTHREADS, 0, st>>>(img, H, W, pitch, thr_img, border, blur_tiled, img_tiled,
                                                                 cand_keys, cand_cap, cand_count, n_img, g.tiles_x, g.tiles_per_img);
  }
  VUS_CHECK_LAUNCH("fast_detect_adaptive_tiled");
  return VUS_OK;
}

extern "C" int vus_fast_detect_retry(const uint8_t* img, int n_img, int H, int W, int pitch, int thr, const int* thr_img,
                                     int max_kp, int border, uint32_t* cand_keys, int cand_cap, int* cand_count,
                                     int* retry_list, int* retry_count, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  VUS_REQUIRE(cand_keys && cand_count && thr_img && retry_list && retry_count, "null buffer");
  VUS_REQUIRE(thr >= 1 && thr <= 254 && max_kp >= 1 && cand_cap >= 1 && border >= 0, "thr=%d max_kp=%d cand_cap=%d border=%d", thr,
              max_kp, cand_cap, border);
  if (n_img == 0) return VUS_OK;
  hipStream_t st = vus::as_stream(stream);
  const TileGrid g = tile_grid(n_img, H, W);
  fast_retry_list_kernel<<<1, 1024, 0, st>>>(thr_img, thr, max_kp, cand_cap, n_img, cand_count, retry_list, retry_count);
  int n_cu = 256;
  {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n_cu < 1)
      n_cu = 256;
  }
  fast_retry_kernel<<<8 * n_cu, NTHREADS, 0, st>>>(img, H, W, pitch, thr, border, cand_keys, cand_cap, cand_count, retry_list,
                                                   retry_count, g.tiles_x, g.tiles_per_img);
  VUS_CHECK_LAUNCH("fast_detect_retry");
  return VUS_OK;
}
