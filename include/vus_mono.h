/* vus_mono.h -- monocular projection factors next to the stereo factors (part of the C ABI of include/vus.h, which
 * includes this file; it can also be included on its own).
 *
 * gtsam::GenericProjectionFactor<Pose3, Point3, Cal3_S2>(measured, model, poseKey, pointKey, K, body_P_sensor): a
 * landmark seen in the left image only.  With the camera at C = X (or X o S with an extrinsic, include/vus_sensor.h) and
 * q = (x, y, z) = Rc^T (p - tc), the calibration K = (fx, fy, s, cx, cy) -- Cal3_S2 DOES use its skew, unlike the
 * StereoCamera of the stereo factor -- predicts
 *
 *   u = cx + fx x/z + s y/z,   v = cy + fy y/z,   residual b = (u - m_u, v - m_v) / sigma_mono,
 *
 * and for z <= 0 (cheirality, judged in the CAMERA frame) the residual is 2 fx / sigma_mono on both rows with zero
 * Jacobians, as the stereo factor has 2 fx / sigma on its three.  With d = 1/z
 *
 *   J = db/dq = 1/sigma_mono [ fx d   s d    -d^2 (fx x + s y) ]     H2 = J Rc^T,   H1_cam = [ J [q]x, -J ]
 *                            [ 0      fy d   -d^2 fy y         ]
 *
 * in the tangent conventions of the stereo factor ([omega, v], H1_body = H1_cam Ad(S^-1)): a monocular observation is
 * the stereo observation without its uR row, with its own calibration and its own sigma.  Both kinds sit in ONE
 * observation list (vus_ba_problem: same L-order / P-order arrays, same duplicate rule -- at most one factor of either
 * kind per pose-landmark pair), told apart by a flag per observation:
 *
 *   is_mono[a] != 0   observation a (L-order, the order of vus_ba_problem.obs_pose / obs_point) is monocular;
 *                     vus_ba_problem.meas row a then holds (u, ignored, v).  The middle slot is never used: it may
 *                     hold anything, NaN included.  A stereo row holds (uL, uR, v) as ever.
 *
 * One calibration and one sigma for all mono factors of a graph, like the one Cal3_S2Stereo and the one sigma of the
 * stereo factors (vus_ba_problem.K / inv_sigma, which keep serving the stereo rows; they must be valid even when
 * every observation is mono).
 *
 * W = H1^T H2 stays 6 x 3 per observation and V, gl, Hpp, gp stay per-variable sums, so every later stage (vus_ba_schur,
 * the band solve, vus_ba_backsub, the retraction, the marginals) is unchanged.  Under a robust model
 * (include/vus_robust.h) a factor's d^2 = |b|^2 is taken over the rows it has (2 for mono, 3 for stereo), the one
 * mEstimator and parameter serve both kinds, and the slots hold what the `_robust` twins report: 0.5 sum w d^2 in the
 * linear slots, sum rho(d) in the nonlinear ones.
 *
 * The entry points below take the arguments of the `_sensor` forms and follow their contract, with
 *   loss     NULL = Gaussian
 *   sensor   NULL = no extrinsic (the poses are the camera's)
 *   mono     must not be NULL.  Validated on the host before any launch: K finite, fx, fy > 0, inv_sigma finite and > 0,
 *            is_mono not NULL when the problem has observations.  A failure is the library's usual negative status.
 * With every flag 0 they compute what vus_ba_* / `_robust` / `_sensor` compute (those stay the ones to call for a graph
 * without mono factors, and launch the same kernels as before).  vus_ba_stereo_weights_mixed returns a weight for EVERY
 * observation, mono included.
 *
 * These entry points have no `_cpu` twin in the oracle library: their CPU statement is the numpy reference of the test
 * suite (tests/mono_ref.py), which evaluates the formulas above per observation beside the oracle's stereo factor. */
#ifndef VUS_MONO_H
#define VUS_MONO_H
#include "vus.h"
#include "vus_robust.h"
#include "vus_sensor.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_ba_mono {
  const unsigned char* is_mono; /* [n_obs] device, L-order: nonzero = GenericProjectionFactor, 0 = GenericStereoFactor3D */
  double K[5];                  /* Cal3_S2 of the mono factors: fx, fy, skew, cx, cy */
  double inv_sigma;             /* 1 / sigma of their Isotropic(2, sigma) model */
} vus_ba_mono;

int vus_ba_linearize_mixed(const vus_ba_problem* P, const double* poses, const double* points, double* W, double* V,
                           double* gl, double* Hpp, double* gp, double* err, double* work, void* stream,
                           const vus_ba_loss* loss, const vus_ba_sensor* sensor, const vus_ba_mono* mono);
int vus_ba_eval_step_mixed(const vus_ba_problem* P, const double* poses, const double* points, const double* dp,
                           const double* dl, double* new_poses, double* new_points, double* out, double* work,
                           void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor, const vus_ba_mono* mono);
int vus_ba_error_mixed(const vus_ba_problem* P, const double* poses, const double* points, double* err, double* work,
                       void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor, const vus_ba_mono* mono);
int vus_ba_stereo_weights_mixed(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses,
                                const double* points, double* w, void* stream, const vus_ba_sensor* sensor,
                                const vus_ba_mono* mono);

#ifdef __cplusplus
}
#endif
#endif /* VUS_MONO_H */
