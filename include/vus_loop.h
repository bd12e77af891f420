/* vus_loop.h -- loop-closure measurements: the relative pose of two stereo keyframes that see the same place, by
 * three-point RANSAC on their metric 3-D points and a Gauss-Newton refit of the left-image reprojection error (part of the
 * C ABI of include/vus.h, which includes this file; it can also be included on its own).
 *
 * Where it sits: vus_hamming_match on the pairing (left(a), left(b)) of two arbitrary keyframes gives match_idx; the stereo
 * matches of both keyframes (what process() leaves in stereo_idx) give every matched keypoint a depth.  This entry point
 * turns that into T_a^-1 T_b with the normal matrix of its refit, ready to become a BetweenFactor<Pose3> (vus_between.h).
 * Which pairs to try is the caller's business (sequence.loop_candidates: pose proximity; sequence.appearance_candidates on
 * vus_keyframe_similarity, vus_retrieval.h: the descriptors alone).
 *
 *   match_idx   int32 [n_pairs, max_kp]   left(a) keypoint i -> left(b) keypoint j of pair c (-1: none)
 *   pair_a, pair_b  int [n_pairs]         DEVICE: frame numbers of pair c; frame f's left image is image 2f, its right 2f+1
 *   stereo_idx  int32 [n_frames, max_kp]  left -> right match of every frame (-1: none)
 *   kp_keys     uint32 [2 n_frames, max_kp], kp_count int [2 n_frames]   as in vus_track_ids: positions are decoded from
 *               the keys (y * W + x in the low 24 bits), counts clamped to max_kp, a negative count an empty list
 *   cam         f64 [5] = fx, fy, cx, cy in pixels of the H x W image, baseline in metres.  A HOST pointer: five scalars
 *               read during the call (the host validates them and derives fb = fx * baseline, thr2 = threshold_px^2)
 *   threshold_px, n_hyp, seed, refine_iters   inlier distance, hypotheses per pair, seed of the samples, refit rounds
 *   T_ab   f64 [n_pairs, 12]   flat12 (R row-major, then t) of T_a^-1 T_b in camera frames: P_a = R Q_b + t
 *   JtJ    f64 [n_pairs, 36]   sum J^T J over the final inliers, tangent order (omega, v) of T Exp(xi), pixel units
 *   rss    f64 [n_pairs]       sum |r|^2 over the final inliers, pixels^2
 *   match_idx_out int32 [n_pairs, max_kp]   match_idx for the final inliers, -1 otherwise; may alias match_idx
 *   info   int32 [n_pairs, 6] = (n, best k, count of the best hypothesis, final inliers, status, refit rounds done)
 *
 * Status -1 (VUS_E_INVALID) with vus_last_error() text, before any launch, for: a null pointer; n_pairs < 1; n_frames < 1;
 * max_kp outside 1..VUS_LOOP_MAX_KP; n_hyp outside 1..VUS_LOOP_MAX_HYP; refine_iters outside 0..VUS_LOOP_MAX_REFINE; H or W
 * below 1; a non-finite or non-positive threshold_px, fx, fy or baseline.
 *
 * ARITHMETIC.  All fp64, operations in the order written, no contraction (the unit is built with -ffp-contract=off).  The
 * numpy restatement of the test suite (tests/loop_ref.py) is the CPU statement of this entry point; it has no `_cpu` twin
 * in the oracle library.  Every integer output (info, match_idx_out) equals the reference's on inputs whose decisions
 * are not within a rounding error of their bounds; T_ab, JtJ and rss differ from it by the summation order and the libm
 * calls of the retraction only.
 *
 * CANDIDATES of pair c = (a, b): slots i in ascending order; nla, nra, nlb, nrb the clamped counts of images 2a, 2a+1,
 * 2b, 2b+1.  Slot i is a candidate when i < nla; j = match_idx[c,i] lies in [0, nlb); sa = stereo_idx[a,i] lies in
 * [0, nra) and sb = stereo_idx[b,j] in [0, nrb); and with (x1, y1) the position of left(a) keypoint i, xr1 the column of
 * right(a) keypoint sa, (x2, y2) and xr2 likewise in b: d1 = x1 - xr1 >= 1 and d2 = x2 - xr2 >= 1 (integers).  The
 * candidates are numbered 0..n-1.  Per candidate
 *
 *   Z1 = fb / d1    P = (((x1 - cx) Z1) / fx,  ((y1 - cy) Z1) / fy,  Z1)        the point in camera a
 *   Z2 = fb / d2    Q = (((x2 - cx) Z2) / fx,  ((y2 - cy) Z2) / fy,  Z2)        the point in camera b
 *   (u, v) = (x2, y2)                                                            its observation in left(b)
 *
 * A pair whose a or b lies outside [0, n_frames), or with a == b, has no candidates (status 1); nothing is indexed with
 * such a value.
 *
 * HYPOTHESIS k = 0..n_hyp-1 (mix = the lowbias32 integer hash of vus_ransac.h, all arithmetic mod 2^32):
 *
 *   h  = mix(seed + 0x9E3779B9 (c + 1))
 *   r1 = mix(h ^ 3k)   r2 = mix(h ^ (3k + 1))   r3 = mix(h ^ (3k + 2))
 *   i  = r1 % n        j = (i + 1 + r2 % (n - 1)) % n
 *   l  = r3 % (n - 2);  if l >= min(i, j): l += 1;  then if l >= max(i, j): l += 1
 *
 * For A = P and for A = Q the triad of the sample:
 *
 *   e1 = A_j - A_i    f = A_l - A_i    c3 = e1 x f  (c3x = e1y fz - e1z fy, c3y = e1z fx - e1x fz, c3z = e1x fy - e1y fx)
 *   n1 = (e1x e1x + e1y e1y) + e1z e1z    n2, n3 likewise of f and c3
 *   degenerate unless n3 > 1e-6 (n1 n2)
 *   e1 <- e1 / sqrt(n1)    e3 = c3 / sqrt(n3)    e2 = e3 x e1
 *
 * With (f1, f2, f3) the triad of P and (e1, e2, e3) that of Q:
 *
 *   R[r][c] = (f1[r] e1[c] + f2[r] e2[c]) + f3[r] e3[c]
 *   t[r]    = P_i[r] - ((R[r][0] Qx_i + R[r][1] Qy_i) + R[r][2] Qz_i)
 *
 * INLIER TEST of a candidate under a model (R, t), without division:
 *
 *   D = P - t     X[c] = (R[0][c] Dx + R[1][c] Dy) + R[2][c] Dz                  X = R^T (P - t): the point of a in camera b
 *   ex = fx Xx - (u - cx) Xz    ey = fy Xy - (v - cy) Xz
 *   inlier = Xz > 0 and (ex ex + ey ey) <= thr2 (Xz Xz)
 *
 * -- the left-image reprojection error of a's 3-D point in camera b.  The right image (disparity) of b enters the
 * hypotheses through Q only: with integer disparities its residual is a staircase that pulls the fit (with the refined ones
 * of vus_stereo_pair_pose_q8 it is not: the second stage of vus_pair_bundle.h takes it into a refit).
 * count_k = number of inliers, or -1 for a degenerate sample.  best = the k of the largest count_k, the lowest k on ties;
 * best = -1 (and the count column -1) if n < 3 or every sample is degenerate.
 *
 * REFIT.  From the best model, refine_iters rounds of: the inlier set of the current model; over it
 *
 *   iz = 1 / Xz    a = fx iz    b = fy iz    px = Xx iz    py = Xy iz
 *   r  = ((fx px + cx) - u,  (fy py + cy) - v)
 *   g2 = -(a px)   h2 = -(b py)
 *   J0 = (-(g2 Xy),  g2 Xx - a Xz,  a Xy,  -a,  0,  -g2)
 *   J1 = (b Xz - h2 Xy,  h2 Xx,  -(b Xx),  0,  -b,  -h2)
 *   H[p][q] += J0[p] J0[q] + J1[p] J1[q]     g[p] += J0[p] r0 + J1[p] r1     rss += r0 r0 + r1 r1
 *
 * (J = dr/dX [ [X]x | -I ]: X(T Exp(xi)) = X + [X]x omega - v to first order); a 6 x 6 Cholesky H = L L^T; delta = H^-1 g;
 * T <- T Exp(-delta), the retraction of the pose kernels (gtsam's Pose3::Expmap).  A round that finds fewer than three
 * inliers (H is then singular, whatever its rounded pivots say) or a pivot that is not > 0 ends the pair with status 3 and
 * the model it entered that round with.  After the last round the inlier set of the final model is
 * taken once more: JtJ = H, rss and match_idx_out are formed on it.  Every slot of every output is written.
 *
 *   status 0 ok;  1 n < 3;  2 no non-degenerate sample;  3 refit solve failed
 *
 * For a non-zero status T_ab is the identity (1, 2) or the last good model (3), JtJ and rss are zero, the final-inlier
 * column is 0 and the output row is all -1.
 *
 * KERNEL.  One workgroup of 256 threads per pair.  The candidates are compacted in index order (ballot + prefix sum) into
 * LDS as P (three doubles), (u, v) as two floats (exact: pixel positions are below 2^24) and d2: 36 B per slot of max_kp --
 * 72,000 B at 2000 (two workgroups per CU), 147,456 B at VUS_LOOP_MAX_KP = 4096, within the 160 KiB a gfx950 workgroup may
 * have; there is no second path.  Q of a sample is recomputed from (u, v, d2) by the statement above.  A lane owns
 * hypotheses k, k + 256, ... and walks all candidates with broadcast LDS reads.  A refit round is one pass in which thread t
 * sums candidates t, t + 256, ... in ascending order, a butterfly over each wave and the four waves added in order -- a
 * fixed tree: two runs give the same bits; no atomics on doubles.  Thread 0 solves.
 *
 * SUB-PIXEL DISPARITIES: vus_stereo_pair_pose_q8.  The same arguments plus disp_q8 int32 [n_frames, max_kp], the refined
 * x_left - x_right of every left keypoint in 1/256 px (what vus_stereo_refine of vus_subpixel.h writes; 0 for an unmatched
 * slot).  Everything above holds with two changes.  The last candidate condition becomes disp_q8[a,i] >= 256 and
 * disp_q8[b,j] >= 256 (the index checks on sa and sb stay; the right keypoints' columns are no longer read), and
 *
 *   Z1 = fb / (disp_q8[a,i] / 256.0)      Z2 = fb / (disp_q8[b,j] / 256.0)
 *
 * (the division by 256.0 is exact).  The 4-byte d2 slot of the LDS layout holds the Q8 integer: the budget per slot and
 * VUS_LOOP_MAX_KP do not move.  disp_q8 = NULL means integer disparities: the call is then vus_stereo_pair_pose, which runs
 * this same code with NULL; disp_q8 = 256 (x_left - x_right) gives its bits too.  The kernel is one text instantiated for
 * the two cases at compile time, so the integer instantiation is the kernel it was before this entry point existed.  The
 * refit's residual stays left-image only.  Validation is that of vus_stereo_pair_pose.
 *
 * NOT IN THESE ENTRY POINTS: a right-image residual in the refit.  It is a second stage behind them, vus_stereo_pair_bundle
 * (vus_pair_bundle.h): both stereo observations of every final inlier, the points left free. */
#ifndef VUS_LOOP_H
#define VUS_LOOP_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_LOOP_MAX_KP 4096
#define VUS_LOOP_MAX_HYP 4096
#define VUS_LOOP_MAX_REFINE 64

int vus_stereo_pair_pose(const int32_t* match_idx,   /* [n_pairs, max_kp] left(a) kp i -> left(b) kp j, -1 none */
                         const int* pair_a, const int* pair_b,   /* [n_pairs] frame numbers; left image 2f, right 2f+1 */
                         const int32_t* stereo_idx,  /* [n_frames, max_kp] left -> right match of every frame */
                         const uint32_t* kp_keys, const int* kp_count, int n_frames, int n_pairs, int max_kp, int H, int W,
                         const double* cam,          /* HOST [5] fx fy cx cy (pixels of the H x W image), baseline (m) */
                         double threshold_px, int n_hyp, uint32_t seed, int refine_iters,
                         double* T_ab,               /* [n_pairs, 12] flat12 of T_a^-1 T_b (camera frames) */
                         double* JtJ,                /* [n_pairs, 36] sum J^T J over the final inliers */
                         double* rss,                /* [n_pairs] sum |r|^2 over the final inliers, pixels^2 */
                         int32_t* match_idx_out,     /* [n_pairs, max_kp] survivors, -1 otherwise; may alias match_idx */
                         int32_t* info,              /* [n_pairs, 6] */
                         void* stream);

int vus_stereo_pair_pose_q8(const int32_t* match_idx, const int* pair_a, const int* pair_b, const int32_t* stereo_idx,
                            const uint32_t* kp_keys, const int* kp_count, int n_frames, int n_pairs, int max_kp, int H, int W,
                            const double* cam, double threshold_px, int n_hyp, uint32_t seed, int refine_iters,
                            const int32_t* disp_q8,     /* [n_frames, max_kp] refined disparities in 1/256 px, may be NULL */
                            double* T_ab, double* JtJ, double* rss, int32_t* match_idx_out, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_LOOP_H */
