/* vus_subpixel.h -- sub-pixel stereo disparities: an integer sum-of-absolute-differences search around every stereo match
 * and an equiangular (V-shaped) line fit of its minimum, in 1/256 px (part of the C ABI of include/vus.h, which includes
 * this file; it can also be included on its own).
 *
 * Where it sits: process() leaves stereo_idx (vus_hamming_match on the pairing (left, right) of every frame), which pairs
 * two FAST corners that were detected independently on integer pixels: x_left - x_right is a whole number.  This entry
 * point measures the right column of every such match on the images themselves.  Its output feeds the u1 column of the
 * CameraMeasurement features (frontend.feature_tracks) and the depths of vus_stereo_pair_pose_q8 (vus_loop.h).
 *
 *   img         uint8 [2 n_frames, H, pitch]   rectified images, row stride `pitch` bytes, W pixels used per row; the left
 *               image of frame f is image 2f, its right image 2f+1
 *   stereo_idx  int32 [n_frames, max_kp]       left keypoint i of frame f -> right keypoint j (-1: none)
 *   kp_keys     uint32 [2 n_frames, max_kp], kp_count int [2 n_frames]   as in vus_track_ids: positions are decoded from
 *               the keys (y * W + x in the low 24 bits), counts clamped to max_kp, a negative count an empty list
 *   half_win    the window is (2 half_win + 1)^2 pixels;  search: shifts s = -search .. search are tried
 *   disp_q8     int32 [n_frames, max_kp]       refined x_left - x_right in 1/256 px
 *   status      uint8 [n_frames, max_kp]       VUS_SUBPIX_OK, VUS_SUBPIX_EDGE or VUS_SUBPIX_NONE
 *
 * Status -1 (VUS_E_INVALID) with vus_last_error() text that names the argument, before any launch, for: a null img,
 * stereo_idx, kp_keys, kp_count, disp_q8 or status; n_frames, H or W below 1; pitch < W; max_kp outside 1..65535; half_win
 * outside 1..VUS_SUBPIX_MAX_HALF_WIN; search outside 1..VUS_SUBPIX_MAX_SEARCH; n_frames * max_kp or an image plane
 * (H * pitch) at or above 2^31.
 *
 * ARITHMETIC.  Integers from the first load to the last store; the numpy restatement of the test suite
 * (tests/subpixel_ref.py) is the CPU statement of this entry point (it has no `_cpu` twin in the oracle library) and every
 * output word EQUALS it.  Integer sums are order-free: two runs give the same bits.
 *
 * SLOT RULE.  nl = min(kp_count[2f], max_kp), nr = min(kp_count[2f+1], max_kp) (a negative count: 0).  Slot (f, i) is
 * matched when i < nl and j = stereo_idx[f,i] lies in [0, nr).  Any other slot gets disp_q8 = 0, status = VUS_SUBPIX_NONE,
 * and nothing is indexed with its values.
 *
 * POSITIONS of a matched slot.  p = kp_keys[2f,i] & VUS_KEY_POS_MASK, yl = p / W, xl = p - yl W; q = kp_keys[2f+1,j] &
 * VUS_KEY_POS_MASK, xr = q - (q / W) W; d0 = xl - xr.  Both windows use row yl: the input is rectified (the matcher's gate
 * lets the two keypoints differ by a few rows; the right keypoint's row is not used).
 *
 * COST.  With cx(x) = min(max(x, 0), W - 1) and cy(y) = min(max(y, 0), H - 1) (replicate border; every coordinate is
 * clamped, or known to need no clamp, before any load, so no key and no table entry can make the kernel read outside an
 * image row), L the left and R the right image of frame f, for s = -search .. search:
 *
 *   cost(s) = sum over dy, dx in [-half_win, half_win] of | L[cy(yl+dy)][cx(xl+dx)] - R[cy(yl+dy)][cx(xr+s+dx)] |
 *
 * The largest cost is 255 * 15^2 = 57375: it fits 16 bits, and 512 times it fits int32.
 *
 * MINIMUM.  s* = the s of the smallest cost, the lowest s on ties (a flat patch therefore ends at -search).
 *
 * EDGE.  s* = -search or s* = +search: status = VUS_SUBPIX_EDGE, disp_q8 = 256 d0 -- the match is kept at its integer
 * value, not dropped.
 *
 * REFINEMENT otherwise, with c- = cost(s* - 1), c0 = cost(s*), c+ = cost(s* + 1):
 *
 *   m = max(c-, c+) - c0
 *   q = 0 if m == 0, else floor((256 (c- - c+) + m) / (2 m))        mathematical floor; q lies in [-128, 128]
 *   disp_q8 = 256 (d0 - s*) - q,  status = VUS_SUBPIX_OK
 *
 * -- the equiangular fit: an absolute-difference cost is V-shaped around its minimum, the two lines through (s* - 1, c-),
 * (s*, c0), (s* + 1, c+) with slopes of equal magnitude meet at s* + (c- - c+) / (2 m); q is 256 times that, rounded half
 * up.  The best right column is xr + s* + q / 256.
 *
 * Every slot of both outputs is written.
 *
 * KERNEL.  Sixteen lanes per slot, four slots per wave, sixteen per workgroup of 256 threads.  Lane r < 2 half_win + 1
 * owns window row r: it loads that row of the left window and the 2 (half_win + search) + 1 bytes of the right strip, four
 * bytes to a register -- unaligned dword loads where the whole-dword span lies inside the image row, clamped byte loads at
 * the borders -- and forms its 2 search + 1 partial sums with the packed byte sum-of-absolute-differences instruction on
 * byte-aligned register pairs.  The partial sums travel two to a register (16 bits each) through four cross-lane
 * exchanges; lane 0 of the group fits and stores.  No LDS, no atomics, no scratch.
 *
 * NOT IN THIS ENTRY POINT: refinement at a keypoint's own pyramid level (in pyramid mode the caller passes the level-0
 * images and the keys' integer level-0 positions); mean or gain removal between the two cameras. */
#ifndef VUS_SUBPIXEL_H
#define VUS_SUBPIXEL_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_SUBPIX_MAX_HALF_WIN 7
#define VUS_SUBPIX_MAX_SEARCH 8

#define VUS_SUBPIX_OK 0
#define VUS_SUBPIX_EDGE 1
#define VUS_SUBPIX_NONE 255

int vus_stereo_refine(const uint8_t* img,        /* [2 n_frames, H, pitch]: left of frame f is image 2f, right 2f+1 */
                      int n_frames, int H, int W, int pitch,
                      const int32_t* stereo_idx, /* [n_frames, max_kp] */
                      const uint32_t* kp_keys, const int* kp_count,   /* [2 n_frames, max_kp], [2 n_frames] */
                      int max_kp, int half_win, int search,
                      int32_t* disp_q8,          /* [n_frames, max_kp] refined x_left - x_right in 1/256 px */
                      uint8_t* status,           /* [n_frames, max_kp] */
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_SUBPIXEL_H */
