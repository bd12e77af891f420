/* vus_rectify.h -- lens undistortion + stereo rectification of raw camera images by a fixed-point remap table (part of
 * the C ABI of include/vus.h, which includes this file; it can also be included on its own).
 *
 * What it replaces: the reference's launch file wires the RAW camera topics into the image-processor nodelet together
 * with a Kalibr-style calibration (distortion model, coefficients, T_cn_cnm1; launch/stereo.launch:5-6, 15, 23-25); the
 * nodelet undistorts on its own.  Here the front end (vus_fast_detect ... vus_hamming_match) takes ideal, row-aligned
 * pinhole images, so raw images pass through vus_rectify_remap first.  The table is built once per calibration on the
 * host (visual_underwater_slam_amd/rectify.py); the two entry points below only read it.  They have no `_cpu` twin in
 * the oracle library: the numpy restatement of the test suite (tests/rectify_ref.py) is their CPU statement, and both
 * are integer arithmetic that equals it bit for bit.
 *
 * MAP.  One 32-bit word per rectified pixel and camera:  map[c][y][x] = (dy << 16) | (dx & 0xFFFF), dx and dy signed
 * 16-bit: the source position MINUS the pixel's own position in 1/32 pixel (Q5).  A real source coordinate u of pixel x
 * is quantised as floor((u - x) * 32 + 0.5).  Relative, because a lens moves a pixel by tens of pixels whatever the
 * image size, so 16 bits hold +-1024 pixels of displacement at any resolution; Q5, because 5 + 5 weight bits times an
 * 8-bit pixel and the rounding term stay far inside 32 bits and 1/32 pixel is below what FAST can tell apart.  Raw and
 * rectified images have the same H x W.
 *
 * REMAP.  For output pixel (x, y) with map word (dx, dy):
 *
 *   sx = (x << 5) + dx      ix = sx >> 5 (arithmetic)      fx = sx & 31          likewise sy, iy, fy from y and dy
 *   x0 = clamp(ix, 0, W-1)  x1 = clamp(ix + 1, 0, W-1)     y0, y1 likewise       (replicate border, as vus_blur7 and
 *                                                                                 vus_resize_bilinear)
 *   out = (p00 (32-fx)(32-fy) + p01 fx (32-fy) + p10 (32-fx) fy + p11 fx fy + 512) >> 10,    p_rc = src[y_r][x_c]
 *
 * Every 16-bit pair is a legal map value: all coordinates are clamped before any load.
 *
 * PLAN (vus_rectify_plan, once per calibration).  The output is cut into tiles of VUS_RECTIFY_TILE_W x
 * VUS_RECTIFY_TILE_H pixels, row-major, tiles_x = ceil(W / 64), tiles_y = ceil(H / 16); tile t of map m is entry
 * m * tiles_x * tiles_y + t.  boxes[entry] = (x0, y0, w, h): the bounding box of the clamped source pixels (x0, x1, y0,
 * y1 above) of the tile's pixels that lie inside the image, by exact integer min / max.  A box FITS when
 *
 *   ((w + 6) & ~3) * h <= VUS_RECTIFY_LDS_BYTES
 *
 * ((w + 6) & ~3 is the row stride of the staged copy: the box's rows start at x0 rounded down to a multiple of 4, so
 * that they are fetched as aligned dwords).  A box that does not fit is written as (0, 0, 0, 0): w = 0 marks it.
 *
 * KERNEL (vus_rectify_remap).  One workgroup of 256 threads per tile, map and group of VUS_RECTIFY_FRAME_GROUP images
 * that share the map (image i uses map i % n_maps: with n_maps = 2 the [2F, H, W] view of a stereo stream); a thread
 * owns 4 consecutive output pixels: one 16-byte map load, decoded once into offsets and weights that stay in registers
 * for the whole group, and one dword store per image.  A tile whose box fits copies the boxes of up to 8 images into
 * LDS side by side (aligned dwords; the LDS array is twice the budget, so at least 2) and gathers the four neighbours
 * of every pixel with LDS byte reads; a tile with w = 0 gathers them from global memory.  The boxes are a schedule
 * only: a workgroup checks that its box lies inside the image, fits, and covers every source pixel of the tile, and
 * takes the global path otherwise, so the output is the REMAP statement above whatever `boxes` holds.  Rows whose
 * address or pitch is not a multiple of 4 are staged and stored bytewise.  Bytes of dst between W and pitch_d are not
 * written.
 *
 *   map    int32 [n_maps, H, W]                     boxes  int32 [n_maps, tiles_y, tiles_x, 4]
 *   src    uint8 [n_img, H, pitch_s] (all n_img * H * pitch_s bytes readable)       dst uint8 [n_img, H, pitch_d]
 *
 * Device pointers; asynchronous on `stream`; nothing is allocated.  Status -1 (VUS_E_INVALID) with vus_last_error()
 * text, before any launch, for: a null pointer; n_maps < 1; n_img < 1 (remap); H or W below 1 or above 32767 (so that
 * a Q5 position fits 21 bits); pitch_s or pitch_d below W; an image of 2^31 bytes or more (H * pitch); `boxes` not
 * 16-byte aligned; n_maps above 65535 or more than 65535 * VUS_RECTIFY_FRAME_GROUP images per map.
 *
 * NOT IN THESE ENTRY POINTS: a raw size different from the rectified size, colour images, building the map on the
 * device, undistorting keypoints instead of images. */
#ifndef VUS_RECTIFY_H
#define VUS_RECTIFY_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_RECTIFY_TILE_W 64
#define VUS_RECTIFY_TILE_H 16
#define VUS_RECTIFY_LDS_BYTES 8192    /* LDS budget of ONE staged source box; a workgroup holds 16 KB (2 to 8 boxes), 8
                                         workgroups -- the wave limit -- 133 of a CU's 160 KB.  The largest box of the
                                         test rig's lens at 720p, which moves pixels by 75, is 66 x 21 pixels = 1.4 KB */
#define VUS_RECTIFY_FRAME_GROUP 32    /* images of one map a workgroup remaps with the same decoded map words */

int vus_rectify_plan(const int32_t* map, int n_maps, int H, int W, int32_t* boxes, void* stream);

int vus_rectify_remap(const uint8_t* src, int n_img, int H, int W, int pitch_s,
                      const int32_t* map, const int32_t* boxes, int n_maps,
                      uint8_t* dst, int pitch_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_RECTIFY_H */
