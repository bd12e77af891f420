/* vus_robust.h -- robust noise models of the stereo factors (part of the C ABI of include/vus.h, which includes this
 * file; it can also be included on its own).
 *
 * gtsam::noiseModel::Robust(mEstimator, Isotropic(3, sigma)) with the default Block reweighting: every
 * GenericStereoFactor3D keeps the isotropic whitening of vus_ba_problem.inv_sigma, b = r / sigma, and is reweighted by
 * one scalar computed from its own Mahalanobis distance d = |b|:
 *
 *   kind                     loss rho(d) = the factor's error                  weight w(d)
 *   VUS_LOSS_GAUSSIAN        d^2 / 2                                           1
 *   VUS_LOSS_HUBER(k)        d^2 / 2 (d <= k),  k d - k^2 / 2                  1 (d <= k),  k / d
 *   VUS_LOSS_CAUCHY(k)       k^2 / 2 log(1 + d^2 / k^2)                        k^2 / (k^2 + d^2)
 *   VUS_LOSS_TUKEY(c)        c^2 / 6 (1 - (1 - d^2/c^2)^3) (d <= c),  c^2 / 6  (1 - d^2/c^2)^2 (d <= c),  0
 *   VUS_LOSS_GEMAN_MCCLURE(c) c^2 / 2  d^2 / (c^2 + d^2)                        c^4 / (c^2 + d^2)^2
 *   VUS_LOSS_WELSCH(c)       c^2 / 2 (1 - exp(-d^2 / c^2))                     exp(-d^2 / c^2)
 *
 * k is in whitened units (Huber k = 1.345 with sigma = 10 px is 13.45 px).  A cheirality observation (z <= 0) has the
 * residual 2 fx / sigma on all three rows and zero Jacobians, as without a robust model, and goes through the same
 * rho / w.  Priors and navigation factors stay Gaussian.
 *
 * The linearisation at x0 takes w = w(d(x0)) per factor and scales the factor's whitened residual and Jacobian rows by
 * sqrt(w) (IRLS): W, V, gl, Hpp, gp then describe the reweighted system and every later stage (vus_ba_schur, the band
 * solve, vus_ba_backsub) is unchanged.  The LINEAR error of that system at a step is 0.5 sum w |b + J delta|^2, which at
 * delta = 0 is 0.5 sum w d^2 -- in general NOT the nonlinear error sum rho(d).  The entry points below report the
 * quadratic value in the linear slots and rho in the nonlinear ones:
 *   vus_ba_linearize_robust   err[0] = 0.5 sum w d^2 (+ priors)                     (linear error at delta = 0)
 *   vus_ba_eval_step_robust   out[0] = 0.5 sum w |b + J delta|^2 (w, b, J at the OLD values, + priors)
 *                             out[1] = sum rho(d) at the new values (+ priors)
 *   vus_ba_error_robust       err[0] = sum rho(d) (+ priors): NonlinearFactorGraph.error()
 * Otherwise they take the arguments of vus_ba_linearize / vus_ba_eval_step / vus_ba_error and follow their contract.
 * A loss of kind VUS_LOSS_GAUSSIAN computes exactly what the entry points without `_robust` compute.
 *
 * These entry points have no `_cpu` twin in the oracle library: their CPU statement is the numpy reference of the test
 * suite, which applies the table above to the oracle's per-observation residuals and Jacobians. */
#ifndef VUS_ROBUST_H
#define VUS_ROBUST_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_LOSS_GAUSSIAN 0
#define VUS_LOSS_HUBER 1
#define VUS_LOSS_CAUCHY 2
#define VUS_LOSS_TUKEY 3
#define VUS_LOSS_GEMAN_MCCLURE 4
#define VUS_LOSS_WELSCH 5

typedef struct vus_ba_loss {
  int kind;     /* VUS_LOSS_* */
  double k;     /* the mEstimator's parameter (k or c), whitened units, finite and > 0 (ignored for VUS_LOSS_GAUSSIAN) */
} vus_ba_loss;

int vus_ba_linearize_robust(const vus_ba_problem* P, const double* poses, const double* points,
                            double* W, double* V, double* gl, double* Hpp, double* gp, double* err,
                            double* work, void* stream, const vus_ba_loss* loss);
int vus_ba_eval_step_robust(const vus_ba_problem* P, const double* poses, const double* points,
                            const double* dp, const double* dl, double* new_poses, double* new_points,
                            double* out, double* work, void* stream, const vus_ba_loss* loss);
int vus_ba_error_robust(const vus_ba_problem* P, const double* poses, const double* points, double* err,
                        double* work, void* stream, const vus_ba_loss* loss);

/* w [n_obs] = the weight w(d) of every stereo observation at (poses, points), L-order (vus_ba_problem.obs_pose /
 * obs_point order): which observations the robust model treats as inliers (w near 1) and which as outliers. */
int vus_ba_stereo_weights(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses, const double* points,
                          double* w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_ROBUST_H */
