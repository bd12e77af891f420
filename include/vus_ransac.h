/* vus_ransac.h -- two-point RANSAC with a known inter-frame rotation on the temporal matches (part of the C ABI of
 * include/vus.h, which includes this file; it can also be included on its own).
 *
 * What it replaces: `ransac_threshold` of the image-processor nodelet (launch/stereo.launch:46, value 3) -- the
 * IMU-aided two-point RANSAC that throws out wrong left(t) -> left(t+1) matches before a feature id is published.  Here
 * it sits between the track matcher (vus_hamming_match on the temporal pairing) and vus_track_ids: a rejected match
 * becomes -1 in the track table, so the two keypoints never share a persistent id.  The test needs the ROTATION between
 * the two frames only (from the gyro: PreintegratedImuMeasurements.deltaRij()); it is independent of translation,
 * odometry drift and landmark depth.
 *
 *   track_idx  int32 [n_frames-1, max_kp]  left(p) -> left(p+1) match of pair p (-1: none), as vus_hamming_match /
 *                                          vus_cross_check leave it
 *   kp_keys    uint32 [2 n_frames, max_kp], kp_count int [2 n_frames]: frame f's left image is image 2f, as in
 *              vus_track_ids.  Positions are decoded, counts clamped to max_kp (negative: an empty list) and a track
 *              index outside [0, count of the next left image) treated as no match exactly as vus_track_ids does, so the
 *              test sees the coordinates that get published.
 *   rot        f64 [n_frames-1, 9]  row-major R_cur_prev of every pair: maps a ray of camera p into camera p+1.  With R_k
 *              the world-from-camera rotation, R_cur_prev = R_{p+1}^T R_p.
 *   cam        f64 [4] = fx, fy, cx, cy in pixels of the H x W image.  A HOST pointer, unlike every other pointer here:
 *              four scalars read during the call (the host validates them and derives tn2 before any launch).
 *   threshold_px, n_hyp, seed   inlier distance in pixels, number of hypotheses per pair, seed of their samples
 *   track_idx_out int32 [n_frames-1, max_kp]  may alias track_idx
 *   info          int32 [n_frames-1, 4] = (n, number surviving, best, number static) per pair
 *
 * Status -1 (VUS_E_INVALID) with vus_last_error() text, before any launch, for: a null pointer; n_frames < 2; max_kp
 * outside 1..8192; n_hyp outside 1..4096; H or W below 1; a non-finite or non-positive threshold_px, fx or fy.
 *
 * ARITHMETIC.  All fp64; only + - x, except the two divisions that normalise a pixel; operations in exactly the order
 * written, no contraction (the unit is built with -ffp-contract=off): the kernel equals the numpy restatement of the test
 * suite (tests/ransac_ref.py) bit for bit.  This entry point has no `_cpu` twin in the oracle library: that numpy
 * reference is its CPU statement.
 *
 * For pair p the matches (i -> j = track_idx[p,i]) are taken in ascending i and numbered 0..n-1.  The host computes
 * tn = threshold_px / ((fx + fy) / 2), tn2 = tn * tn.  With (x1, y1) the position of keypoint i in left(p), (x2, y2) that
 * of keypoint j in left(p+1) and r0..r8 = rot[p], per match:
 *
 *   a1 = (x1 - cx) / fx   b1 = (y1 - cy) / fy   a2 = (x2 - cx) / fx   b2 = (y2 - cy) / fy
 *   X = (r0 a1 + r1 b1) + r2     Y = (r3 a1 + r4 b1) + r5     Z = (r6 a1 + r7 b1) + r8
 *   front  = Z > 0
 *   dx = a2 Z - X    dy = b2 Z - Y
 *   static = front and (dx dx + dy dy) <= tn2 (Z Z)
 *   m = (Y - Z b2,  Z a2 - X,  X b2 - Y a2)                                   (p1 x p2, homogeneous)
 *
 * Hypothesis k = 0..n_hyp-1 (mix = the lowbias32 integer hash, all arithmetic mod 2^32):
 *
 *   a  = mix(seed + 0x9E3779B9 (p + 1))
 *   r1 = mix(a ^ 2k)     r2 = mix(a ^ (2k + 1))
 *   i  = r1 % n          j = (i + 1 + r2 % (n - 1)) % n
 *   t  = m_i x m_j:  tx = my_i mz_j - mz_i my_j   ty = mz_i mx_j - mx_i mz_j   tz = mx_i my_j - my_i mx_j
 *
 * and for every match, l = t x (X, Y, Z):
 *
 *   lx = ty Z - tz Y    ly = tz X - tx Z    lz = tx Y - ty X
 *   e  = (lx a2 + ly b2) + lz            q = lx lx + ly ly
 *   inlier = front and (static or (q > 0 and e e <= tn2 q))
 *
 * -- the distance of p2 from the epipolar line through the rotated p1, in pixels, without division or square root.  The
 * line passes through the rotated p1, so a `static` match (one that moved less than the threshold once the rotation is
 * taken out) is an inlier of every model: a standing camera, where t is exactly 0, does not reject everything.
 * count_k = number of inliers, or -1 if sample i or j is not `front`.  best = the k of the largest count_k, the lowest k
 * on ties; best = -1 if n < 2 or the largest count is negative (no model: every `front` match survives).
 *
 *   track_idx_out[p,i] = track_idx[p,i] for the survivors, -1 for everything else (matches that are not `front`,
 *   invalid indices, slots at or beyond the clamped count of left(p)).  Every slot is written.
 *
 * KERNEL.  One workgroup of 256 threads per pair; the matches are compacted in index order (ballot + prefix sum) into
 * LDS as (X, Y, Z, a2, b2) plus one `static` bit (m and `front` are recomputed from these with the same operations); a
 * lane owns hypothesis k, k + 256, ... and walks all n matches with broadcast LDS reads.  Up to
 * VUS_RANSAC_LDS_MATCHES matches of a pair live in LDS that way (40 B each: two workgroups per CU at max_kp <= 2000).  A
 * pair with MORE matches keeps only the two packed positions per match in LDS (8 B) and recomputes the per-match values
 * from them for every hypothesis -- the same operations in the same order, so the result is identical, at several times
 * the cost.
 *
 * NOT IN THIS ENTRY POINT: a least-squares refit of the model over its inliers, a maximum-displacement pre-gate, and the
 * pyramid's sub-pixel positions (kp_xy_q4): the test uses the integer level-0 positions of the keys. */
#ifndef VUS_RANSAC_H
#define VUS_RANSAC_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_RANSAC_MAX_KP 8192
#define VUS_RANSAC_MAX_HYP 4096
#define VUS_RANSAC_LDS_MATCHES 2000   /* pairs with more matches take the recompute path */

int vus_two_point_ransac(const int32_t* track_idx, const uint32_t* kp_keys, const int* kp_count,
                         int n_frames, int max_kp, int H, int W,
                         const double* rot,   /* [n_frames-1, 9] row-major R_cur_prev */
                         const double* cam,   /* [4] fx, fy, cx, cy in pixels of the H x W image; HOST pointer */
                         double threshold_px, int n_hyp, uint32_t seed,
                         int32_t* track_idx_out,  /* [n_frames-1, max_kp]; may alias track_idx */
                         int32_t* info,           /* [n_frames-1, 4] */
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_RANSAC_H */
