/* vus_tiled.h -- block-tiled image planes for the single-level front-end (included on its own; not part of vus.h).
 *
 * The orientation + rBRIEF stage gathers, per keypoint, a 31-row patch of the image and a 37-row patch of its 7 x 7
 * smoothing.  In row-major planes every patch row touches one or two 128-byte lines of its own (~70 L1 <- L2 requests
 * per keypoint).  In a block-tiled plane a patch of 40 x 31 bytes lies in a few dozen 128-byte blocks.
 *
 * Layout: blocks of VUS_TILE_BW x VUS_TILE_BH = 16 x 8 pixels, each block one contiguous 128-byte line (16 bytes per
 * pixel row, 8 rows), blocks in raster order.  Pixel (y, x) of an H x W plane sits at byte vus_tiled_offset(y, x, W);
 * image n of a batch starts at byte n * H * W.  The tiled entry points take planes whose W is a multiple of 16 and H a
 * multiple of 8 only (every block whole, no padding pixels) and reject other sizes with VUS_E_INVALID: callers keep
 * the row-major entry points for those.
 *
 * All pointers are device pointers, every call is asynchronous on `stream`, allocates nothing and returns 0 or a
 * negative VUS_E_* code, as in vus.h.
 */
#ifndef VUS_TILED_H
#define VUS_TILED_H
#include "vus.h"

#define VUS_TILE_BW 16
#define VUS_TILE_BH 8

#if defined(__HIPCC__)
#define VUS_TILED_QUAL __host__ __device__ static inline
#else
#define VUS_TILED_QUAL static inline
#endif

/* byte offset of pixel (y, x) inside one block-tiled plane of width W (W % 16 == 0; 0 <= y, 0 <= x < W; a plane of up
 * to 2^24 pixels, as everywhere in vus.h, so the offset fits 32 bits) */
VUS_TILED_QUAL unsigned vus_tiled_offset(int y, int x, int W) {
  const unsigned uy = (unsigned)y, ux = (unsigned)x;
  return (uy / VUS_TILE_BH) * ((unsigned)W * VUS_TILE_BH) + (ux / VUS_TILE_BW) * (VUS_TILE_BW * VUS_TILE_BH) +
         (uy % VUS_TILE_BH) * VUS_TILE_BW + ux % VUS_TILE_BW;
}

#ifdef __cplusplus
extern "C" {
#endif

/* vus_fast_detect_adaptive with block-tiled outputs: the same candidate lists, counts and overflow semantics, and
 * instead of the row-major smoothing
 *   blur_tiled [n_img, H * W]  the 7 x 7 smoothing (vus_fast_detect's blur_out), block-tiled
 *   img_tiled  [n_img, H * W]  the input images themselves, block-tiled
 * Both planes depend on the images only and are complete after this call: vus_fast_detect_retry (which re-detects
 * images at fast_threshold) does not touch them.  Both 16-byte aligned; W % 16 == 0, H % 8 == 0. */
int vus_fast_detect_adaptive_tiled(const uint8_t* img, int n_img, int H, int W, int pitch, const int* thr_img, int border,
                                   uint8_t* blur_tiled, uint8_t* img_tiled, uint32_t* cand_keys, int cand_cap,
                                   int* cand_count, void* stream);

/* vus_orient_rbrief_ordered (order may be null: vus_orient_rbrief) on the block-tiled planes of
 * vus_fast_detect_adaptive_tiled: bit-identical descriptors and angles. */
int vus_orient_rbrief_tiled(const uint8_t* img_tiled, const uint8_t* blur_tiled, int n_img, int H, int W,
                            const uint32_t* kp_keys, const int* kp_count, int max_kp, const int* order,
                            uint64_t* desc_out, uint8_t* angle_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
