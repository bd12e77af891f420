/* vus_clahe.h -- contrast-limited adaptive histogram equalisation (CLAHE) of 8-bit images in front of the detector (part
 * of the C ABI of include/vus.h, which includes this file; it can also be included on its own).
 *
 * Why: under water backscatter adds a veiling light and the vehicle's lamp lights a cone that falls off towards the image
 * border; the detector's fixed threshold (vus_fast_detect*, fast_threshold = 10) finds next to nothing on such frames.
 * CLAHE is the photometric counterpart of the geometric input stage of vus_rectify.h: rectified frames pass through
 * vus_clahe_luts + vus_clahe_apply before the front end sees them.  The two entry points have no `_cpu` twin in the oracle
 * library: the numpy restatement of the test suite (tests/clahe_ref.py) is their CPU statement, and both are integer
 * arithmetic that equals it bit for bit.  All divisions below are integer divisions of non-negative numbers unless a
 * floor is written out.
 *
 * TILES AND PADDING.  Parameters tiles_x, tiles_y (1 .. 32 each), an integer clip >= 0, an image of H x W 8-bit pixels.
 * tw = ceil(W / tiles_x), th = ceil(H / tiles_y), T = tw * th.  Tile (j, i) covers rows [j th, (j + 1) th) and columns
 * [i tw, (i + 1) tw) of the PADDED image: a padded row r >= H reads row 2 (H - 1) - r (reflect-101), columns likewise --
 * OpenCV's copyMakeBorder padding for sizes that do not divide.  A tile may lie wholly in the padding; it is still
 * defined.  The call is refused unless
 *
 *   tiles_y th - H <= H - 1,    tiles_x tw - W <= W - 1,    T <= 2^22,    H, W <= 32767.
 *
 * LUT PER TILE.
 *   1. h[0..255]: the histogram of the tile's T padded pixels.
 *   2. If clip > 0:  excess = sum_b max(h[b] - clip, 0);  h[b] = min(h[b], clip);  batch = excess / 256, r = excess % 256;
 *      every bin gets + batch;  if r > 0: step = max(256 / r, 1) and bin b gets + 1 iff b % step == 0 and b / step < r.
 *      (OpenCV's single redistribution pass: bins may end above clip.)
 *   3. c[b] = h[0] + ... + h[b];  lut[b] = (c[b] 255 + T / 2) / T.  The bins still sum to T, so lut[255] = 255 always.
 *
 * INTERPOLATION.  Per column x:  p = 2 x - tw;  t1 = floor(p / (2 tw)) (can be -1);  a = p - t1 2 tw, in [0, 2 tw);
 *   wx = (a 256 + tw) / (2 tw), in [0, 256];  x1 = clamp(t1, 0, tiles_x - 1), x2 = clamp(t1 + 1, 0, tiles_x - 1).
 * Rows likewise with th: y1, y2, wy.  For a pixel of value v:
 *
 *   out = (lut[y1][x1][v] (256 - wx)(256 - wy) + lut[y1][x2][v] wx (256 - wy)
 *        + lut[y2][x1][v] (256 - wx) wy        + lut[y2][x2][v] wx wy          + 32768) >> 16
 *
 * tiles = 1 x 1 with clip = 0 is plain global histogram equalisation; the statement stays within 2 grey levels of the
 * float32 textbook / OpenCV formula (lutScale = 255 / T, round to nearest even, weights x / tw - 0.5): one level from
 * the Q8 weights, one from the rounding.
 *
 * HOST SIDE.  A clip LIMIT (OpenCV's clipLimit, 4.0 here) becomes clip = max(1, int(clip_limit * T / 256)) for
 * clip_limit > 0, else 0, in double precision (visual_underwater_slam_amd/clahe.py, clip_count).  The C ABI takes the
 * integer.
 *
 * KERNELS.  vus_clahe_luts: one workgroup of 256 threads per (image, tile); the tile's rows are read as aligned 16-byte
 * vectors (dwords or bytes where the image or its pitch is not aligned that far); a tile of the last tile row or column
 * reads its padding as the reflected rows and the reflected column span of the image itself.  The histogram lives in LDS
 * as VUS_CLAHE_HIST_COPIES interleaved copies, bin b of copy c at dword b * 16 + c, lane l adding to copy l & 15: of the
 * 32 lanes that add in one cycle at most two meet on an address, whatever the image holds (a murky or constant tile puts
 * every lane on one or two bins; one histogram per wave then takes 3.6 x as long, profiles/clahe.md).  One wave clips,
 * redistributes, scans and writes the 256 bytes.  vus_clahe_apply: the image is cut at the tile CENTRES (ceil(tw / 2) +
 * k tw, ceil(th / 2) + k th), so that a workgroup's pixels share x1, x2, y1, y2; the four LUTs are staged in LDS as one
 * dword per grey level, a thread owns 4 consecutive pixels of a row (dword load, one LDS read per pixel, dword store;
 * bytewise at odd addresses), wx costs one division per thread and wy one per row of the workgroup, and the blend is two
 * packed 16-bit multiply-adds and a 16-bit dot product that equal the sum above exactly.
 *
 *   src   uint8 [n_img, H, pitch_s] (all n_img * H * pitch_s bytes readable)      dst  uint8 [n_img, H, pitch_d]
 *   luts  uint8 [n_img, tiles_y, tiles_x, 256]
 *
 * Device pointers; asynchronous on `stream`; nothing is allocated.  dst may equal src with pitch_d == pitch_s (in
 * place); any other overlap is undefined.  Bytes of dst between W and pitch_d are not written.  Status -1
 * (VUS_E_INVALID) with vus_last_error() text, before any launch, for: a null pointer; n_img < 1; H or W below 1 or above
 * 32767; a pitch below W; an image of 2^31 bytes or more (H * pitch); tiles_x or tiles_y outside 1 .. 32; clip < 0; the
 * padding condition or the T limit above.
 *
 * NOT IN THESE ENTRY POINTS: 16-bit or colour input, CLAHE fused into the remap or the detector, per-level CLAHE in the
 * pyramid, dehazing or colour correction. */
#ifndef VUS_CLAHE_H
#define VUS_CLAHE_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_CLAHE_MAX_TILES 32        /* per axis */
#define VUS_CLAHE_MAX_TILE_PIXELS (1 << 22)   /* T: c[b] * 255 + T / 2 stays inside 32 bits */
#define VUS_CLAHE_HIST_COPIES 16      /* interleaved LDS histograms of a workgroup: 16 KB */

int vus_clahe_luts(const uint8_t* src, int n_img, int H, int W, int pitch_s,
                   int tiles_x, int tiles_y, int clip, uint8_t* luts, void* stream);

int vus_clahe_apply(const uint8_t* src, int n_img, int H, int W, int pitch_s,
                    const uint8_t* luts, int tiles_x, int tiles_y,
                    uint8_t* dst, int pitch_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_CLAHE_H */
