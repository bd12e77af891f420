/* vus_combined_imu.h -- GTSAM's CombinedImuFactor in the per-keyframe-bias layout (part of the C ABI of include/vus.h, which
 * includes this file; it can also be included on its own):
 *   CombinedImuFactor(X(i), V(i), X(i+1), V(i+1), B(i), B(i+1), pim)
 * ONE 15-row factor for the preintegrated measurement and the bias drift of the same interval, whitened with the full
 * 15 x 15 covariance that vus_imu_preintegrate_combined propagates.  An add-on to the factors of include/vus_nav_bias.h
 * with its own buffers: ImuFactor and BetweenFactorConstantBias on other intervals stay in vus_navb_factors.  All pointers
 * are device pointers (but those of vus_imu_preintegrate_combined, a host function), every call is asynchronous on `stream`,
 * allocates nothing and returns 0 or a negative VUS_E_* code, as in vus.h.  The arguments are checked on the host before
 * anything is launched; the index arrays are read back for that (one blocking copy per array and call).
 *
 * Residual (15): r = [ r_imu (9: theta, p, v) ; b_j - b_i (6: acc, gyro) ], r_imu the ImuFactor residual at the bias B(i)
 * with the first-order bias correction of the 148-double record.  Jacobian (15 x 30), columns X_i(6) V_i(3) X_j(6) V_j(3)
 * B_i(6) B_j(6): rows 0..8 the ImuFactor Jacobian in its 24 columns and zero in B_j, rows 9..14 -I in B_i and +I in B_j.
 * Whitened by W [15, 15] = L^-1, Sigma = L L^T, error order (theta, p, v, b_a, b_g).
 *
 * Nodes (vus_ba_problem.pose_stride = 3): X_i 3i, V_i 3i+1, B_i 3i+2, X_j 3i+3, V_j 3i+4, B_j 3i+5.  The joint whitening
 * couples B_j with X_i, five nodes apart: the blocks fill the 6 innermost block diagonals and the node band is at least
 * min(5, n_nodes - 1).
 */
#ifndef VUS_COMBINED_IMU_H
#define VUS_COMBINED_IMU_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_cimu_factors {
  int n;               /* factors, >= 1 */
  const int* i;        /* [n] keyframe of the earlier state, 0 <= i < n_poses - 1 */
  const int* j;        /* [n] = i + 1 */
  const double* pim;   /* [n,148] preintegration records, as vus_nav_factors.imu_pim */
  const double* W;     /* [n,225] whitening matrices, row-major 15 x 15 */
  double gravity[3];
} vus_cimu_factors;

/* HOST function.  vus_imu_preintegrate with the bias random walk: the n samples {acc[3], gyro[3], dt} are integrated on
 * top of the state held by the 148-double record `pim` (means, bias Jacobians and its 9 x 9 covariance exactly as
 * vus_imu_preintegrate leaves them) and by cov15 [225], the 15 x 15 covariance in the error order (theta, p, v, b_a, b_g),
 * all zero for a fresh interval.  Per sample Sigma <- F Sigma F^T + Q with F = [[A, G], [0, I6]]: A the 9 x 9 matrix of
 * vus_imu_preintegrate, G (9 x 6) = [B | C] the per-sample sensitivity to the bias error (b_a columns: dt^2/2 dR on the p
 * rows and dt dR on the v rows; b_g columns: dt Jr on the theta rows), Q the 9 x 9 noise of vus_imu_preintegrate plus
 * bias_acc_cov dt and bias_omega_cov dt on the two bias blocks.  With both bias covariances zero the top-left 9 x 9 of
 * cov15 is the record's covariance bit for bit.  The recursion carries the p and v errors in the frame of keyframe i, as the
 * record's 9 x 9 does; the residual has them in the frame of keyframe j (r_p = R_j^T (..), r_v = R_j^T (..)), so its
 * covariance is T cov15 T^T with T = diag(I, dR^T, dR^T, I, I), dR the record's rotation.  whiten (may be null): W = L^-1
 * with T cov15 T^T = L L^T, row-major 15 x 15; VUS_E_INVALID ("not positive definite", nothing but finite numbers written)
 * if that is not positive definite, as when a bias covariance is zero. */
int vus_imu_preintegrate_combined(double* pim, double* cov15, const double* samples, int n, const double* acc_cov,
                                  const double* gyro_cov, const double* int_cov, const double* bias_acc_cov,
                                  const double* bias_omega_cov, double* whiten);

/* doubles of `work` for the entry points below */
long long vus_cimu_work_doubles(const vus_cimu_factors* F);

/* Residuals and Jacobians of every factor at (poses [n_poses,12], vels [n_poses,3], biases [n_poses,6]), accumulated into
 *   Scimu [3 n_poses, 6, 36]  blocks (node, node - s), s = 0..5   (undamped; zeroed by the call before it accumulates)
 *   gcimu [6 * 3 n_poses]     node gradient
 *   err   [1]                 0.5 * sum |whitened residual|^2
 * One workgroup per factor; the blocks receive their addends with f64 atomics (a pose block two factors'), so two runs
 * agree to ~1e-16 relative, not bitwise. */
int vus_cimu_linearize(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels, const double* biases,
                       double* Scimu, double* gcimu, double* err, double* work, void* stream);

/* Per lambda, after vus_navb_assemble (which damps the velocity and bias nodes): Sband += Scimu on the 6 innermost block
 * diagonals, gs += gcimu.  n_nodes = 3 n_poses, min(5, n_nodes - 1) <= band < n_nodes. */
int vus_cimu_assemble(int n_nodes, int band, const double* Scimu, const double* gcimu, double* Sband, double* gs,
                      void* stream);

/* out[0] = linearised error of the factors at the node step dc [6 * 3 n_poses] (Jacobians at the OLD values), out[1] =
 * their error at (new_poses, new_vels, new_biases), which vus_ba_eval_step and vus_navb_eval_step have written. */
int vus_cimu_eval_step(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels, const double* biases,
                       const double* dc, const double* new_poses, const double* new_vels, const double* new_biases,
                       double* out, double* work, void* stream);

/* err[0] = error of the factors at (poses, vels, biases). */
int vus_cimu_error(const vus_cimu_factors* F, int n_poses, const double* poses, const double* vels, const double* biases,
                   double* err, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_COMBINED_IMU_H */
