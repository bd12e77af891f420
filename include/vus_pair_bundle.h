/* vus_pair_bundle.h -- the second stage of a loop-closure measurement: a two-view refit behind vus_stereo_pair_pose(_q8)
 * (vus_loop.h) in which the inlier points are left free and BOTH stereo observations of every point enter, (x, y, d) in
 * keyframe a and in keyframe b; the pose comes from the Schur-reduced 6 x 6 system (part of the C ABI of include/vus.h,
 * which includes this file; it can also be included on its own).
 *
 * Why: the refit of vus_loop.h takes a's depths as exact and never looks at b's disparity.  Its pose inherits the depth
 * error of every point and its covariance does not know of it.  Here a point's depth is an unknown that both disparities
 * (and both left positions) measure, so refined disparities (vus_subpixel.h) pay off, and S is the information of the pose
 * with the disparity noise in it.
 *
 *   match_in    int32 [n_pairs, max_kp]   stage one's match_idx_out: its final inliers (any match table is accepted)
 *   pair_a, pair_b, stereo_idx, kp_keys, kp_count, n_frames, n_pairs, max_kp, H, W, cam (HOST [5])   as in vus_loop.h
 *   disp_q8     int32 [n_frames, max_kp]  refined disparities in 1/256 px, or NULL: the integer disparities of the keys
 *   T_in        f64 [n_pairs, 12]         stage one's T_ab: where the refit starts
 *   info_in     int32 [n_pairs, 6]        stage one's info; only column 4 (its status) is read
 *   sigma_uv_px, sigma_disp_px            standard deviations of a left pixel position and of a disparity, pixels
 *   gate        a point takes part while its whitened error is at most gate (in sigmas); iters: rounds
 *   T_ab   f64 [n_pairs, 12]      flat12 of T_a^-1 T_b in camera frames: P_a = R Q_b + t
 *   S      f64 [n_pairs, 36]      the reduced normal matrix of the pose over the final active points, tangent order (omega, v)
 *                                 of T Exp(xi); WHITENED: S^-1 is the covariance of the pose at unit residual scale
 *   chi2   f64 [n_pairs]          sum of the whitened squared residuals over the final active points (6 per point)
 *   points f64 [n_pairs, max_kp, 3]   the refined point of every final active slot in camera a's frame, zero elsewhere
 *   match_idx_out int32 [n_pairs, max_kp]   match_in for the final active points, -1 otherwise; may alias match_in
 *   info   int32 [n_pairs, 6] = (n, active points in round 0, final active points, status, rounds done, 0)
 *
 * Status -1 (VUS_E_INVALID) with vus_last_error() text, before any launch, for: a null pointer (disp_q8 excepted);
 * n_pairs < 1; n_frames < 1; max_kp outside 1..VUS_LOOP_MAX_KP; iters outside 0..VUS_LOOP_MAX_REFINE; H or W below 1; a
 * non-finite or non-positive sigma_uv_px, sigma_disp_px, gate, fx, fy or baseline.
 *
 * ARITHMETIC.  All fp64, operations in the order written, no contraction (the unit is built with -ffp-contract=off).  The
 * numpy restatement of the test suite (tests/pair_bundle_ref.py) is the CPU statement of this entry point.  Every integer
 * output equals the reference's on inputs whose decisions are not within a rounding error of their bounds; T_ab, S, chi2
 * and points differ from it by the order of the sums and the libm calls of the retraction only.
 *
 * CANDIDATES of pair c = (a, b): the rule of vus_loop.h applied to match_in -- the same index, count and disparity checks,
 * with disp_q8 the Q8 rule (disp_q8[a,i] >= 256 and disp_q8[b,j] >= 256) -- numbered 0..n-1 in ascending slot order.  A pair
 * whose a or b lies outside [0, n_frames), or with a == b, indexes nothing and has no candidates.
 *
 * PASS-THROUGH.  A pair with info_in[c][4] != 0 is not refitted: status 4, T_ab = T_in, S, chi2 and points zero, the
 * output row all -1, info = (0, 0, 0, 4, 0, 0).
 *
 * OBSERVATIONS of a candidate: za = (x1, y1, d1), zb = (x2, y2, d2), positions of the two left keypoints and the
 * disparities, each d the integer of vus_loop.h or disp_q8 / 256.0 (exact).
 * WEIGHTS w = (wu, wu, wd), wu = 1 / (sigma_uv_px sigma_uv_px), wd = 1 / (sigma_disp_px sigma_disp_px); g2 = gate gate.
 * STATE.  T starts at T_in.  p_i starts at the triangulation of za_i, the P of vus_loop.h:
 *   Z = fb / d1    p = (((x1 - cx) Z) / fx, ((y1 - cy) Z) / fy, Z)
 *
 * ONE ROUND, per candidate:
 *
 *   D = p - t      X[c] = (R[0][c] Dx + R[1][c] Dy) + R[2][c] Dz                  X = R^T (p - t): the point in camera b
 *   of Y = p with z = za, and of Y = X with z = zb:
 *     iz = 1 / Yz    e = fb iz    px = Yx iz    py = Yy iz    a = fx iz    b = fy iz
 *     r = ((fx px + cx) - z0,  (fy py + cy) - z1,  e - z2)                        r = pi(Y) - z
 *     g = -(a px)    h = -(b py)    k = -(e iz)                                    D(Y) = [a 0 g; 0 b h; 0 0 k]
 *   e2 = ((wu ra0 ra0 + wu ra1 ra1) + wd ra2 ra2) + ((wu rb0 rb0 + wu rb1 rb1) + wd rb2 rb2)   (products left to right)
 *   active = pz > 0 and Xz > 0 and e2 <= g2 and the three pivots of A below are > 0
 *
 * The active set is decided anew every round from the current state; an inactive point keeps its p.  Jacobians by
 * residual row k = 0, 1, 2, (a, b, g, h, k) those of X unless marked:
 *
 *   Ja = D(p)                          the (a, b, g, h, k) of p
 *   Jp[0][c] = a R[c][0] + g R[c][2]    Jp[1][c] = b R[c][1] + h R[c][2]    Jp[2][c] = k R[c][2]                 D(X) R^T
 *   Jt[0] = (-(g Xy),  g Xx - a Xz,  a Xy,  -a,  0,  -g)                                               D(X) [ [X]x | -I ]
 *   Jt[1] = (b Xz - h Xy,  h Xx,  -(b Xx),  0,  -b,  -h)
 *   Jt[2] = (-(k Xy),  k Xx,  0,  0,  0,  -k)
 *
 * (X(T Exp(xi)) = X + [X]x omega - v to first order: the tangent of the refit of vus_loop.h, whose J0 and J1 are Jt[0]
 * and Jt[1]).  With <L, M>[r][c] = ((w0 L[0][r]) M[0][c] + (w1 L[1][r]) M[1][c]) + (w2 L[2][r]) M[2][c], and likewise
 * against a residual:
 *
 *   A = <Ja, Ja> + <Jp, Jp>    B = <Jp, Jt>    C = <Jt, Jt>    gp = <Ja, ra> + <Jp, rb>    gt = <Jt, rb>
 *
 * A = L L^T (3 x 3 Cholesky, a pivot that is not > 0 makes the point inactive for the round); Y = A^-1 B and yp = A^-1 gp
 * by forward and back substitution;
 *
 *   S[r][c] += C[r][c] - ((B[0][r] Y[0][c] + B[1][r] Y[1][c]) + B[2][r] Y[2][c])       (upper triangle, mirrored at the end)
 *   g[r]    += gt[r]   - ((B[0][r] yp[0]   + B[1][r] yp[1])   + B[2][r] yp[2])         chi2 += e2
 *
 * over the active points.  Fewer than three active points (S is then singular, whatever its rounded pivots say) or a
 * pivot of the 6 x 6 Cholesky S = L L^T that is not > 0 ends the pair with status 3 and the T it entered the round with.
 * Otherwise delta = S^-1 g;  for every active point  p <- p - A^-1 (gp - B delta)  (blocks of the state before the
 * step);  T <- T Exp(-delta), the retraction of the pose kernels (gtsam's Pose3::Expmap).
 *
 * After the last round the active set of the final state is taken once more: S, chi2, match_idx_out and points are formed
 * on it (with iters = 0 that is the only pass, on the state described under STATE).  Every slot of every output is written.
 *
 *   status 0 ok;  1 n < 3;  3 solve failed;  4 passed through (2 is not used: it is stage one's)
 *
 * For a non-zero status T_ab is T_in (1, 4) or the last good model (3); S, chi2 and points are zero, the final-active
 * column is 0 and the output row is all -1.
 *
 * Points on one line, or copies of one point, make S singular in exact arithmetic; its later pivots are then rounding
 * errors of either sign, and whether such a pair ends with status 3 or with some pose along the free direction is not
 * defined.  Stage one refuses such sets (its status 2) and they are passed through.
 *
 * KERNEL.  One workgroup of 256 threads per pair.  The candidates are compacted in slot order (ballot + prefix sum) into
 * LDS as what a slot needs to rebuild its observations: the two key positions, the two disparity integers and the slot
 * number, 20 B per slot of max_kp -- 40,000 B at 2000, 81,920 B at VUS_LOOP_MAX_KP = 4096, next to 1.1 KiB of static LDS,
 * within the 160 KiB a gfx950 workgroup may have; there is no second path.  Thread t owns candidates t, t + 256, ...  A
 * point's p lives in `points` between the passes: only its owner reads and writes it, so the output is the workspace.
 * A round is one pass over a thread's own points (blocks formed and eliminated in registers), the reduction of the 21 + 6
 * + 1 sums by the fixed tree of vus_stereo_pair_pose (ascending per thread, a butterfly per wave, the four waves added in
 * order: two runs give the same bits; no atomics on doubles), the solve on thread 0, and a second pass over the same
 * points that recomputes their blocks for the back-substitution.
 *
 * NOT IN THIS ENTRY POINT: hypotheses scored with this residual; more than two views; a robust loss (the gate is the
 * rejection rule). */
#ifndef VUS_PAIR_BUNDLE_H
#define VUS_PAIR_BUNDLE_H
#include "vus.h"
#include "vus_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

int vus_stereo_pair_bundle(const int32_t* match_in,    /* [n_pairs, max_kp] stage one's match_idx_out */
                           const int* pair_a, const int* pair_b, const int32_t* stereo_idx, const uint32_t* kp_keys,
                           const int* kp_count, int n_frames, int n_pairs, int max_kp, int H, int W,
                           const double* cam,          /* HOST [5] fx fy cx cy (pixels of the H x W image), baseline (m) */
                           const int32_t* disp_q8,     /* [n_frames, max_kp] refined disparities in 1/256 px, may be NULL */
                           const double* T_in,         /* [n_pairs, 12] stage one's T_ab */
                           const int32_t* info_in,     /* [n_pairs, 6] stage one's info */
                           double sigma_uv_px, double sigma_disp_px, double gate, int iters,
                           double* T_ab,               /* [n_pairs, 12] */
                           double* S,                  /* [n_pairs, 36] reduced, whitened normal matrix of the pose */
                           double* chi2,               /* [n_pairs] */
                           double* points,             /* [n_pairs, max_kp, 3] f64, camera a's frame; also the workspace */
                           int32_t* match_idx_out,     /* [n_pairs, max_kp] may alias match_in */
                           int32_t* info,              /* [n_pairs, 6] */
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_PAIR_BUNDLE_H */
