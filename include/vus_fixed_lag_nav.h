/* vus_fixed_lag_nav.h -- the fixed-lag prior of an INERTIAL window (part of the C ABI of include/vus.h, which includes this
 * file; it can also be included on its own): a dense Gaussian prior over the pose, velocity and IMU bias of consecutive
 * keyframes in the per-keyframe-bias layout of include/vus_nav_bias.h (the add-on family `nav_window_prior`), and the
 * compaction that turns what vus_ba_band_marginalize (include/vus_fixed_lag.h) leaves of such a system into one.
 * All pointers are device pointers, every call is asynchronous on `stream`, allocates nothing and returns 0 or a negative
 * VUS_E_* code, as in vus.h.  Every argument is checked on the host before anything is launched.
 *
 * Semantics (GTSAM's LinearContainerFactor holding a HessianFactor over X(i), V(i), B(i), recalled, not checked against an
 * upstream build): keyframe i of the window, first <= first + i < first + m, contributes 15 values to the tangent vector
 *   delta[15 i ..]      = Local(x0_i, x_i) = Log(x0_i^-1 x_i)   6, tangent order (omega, v)
 *   delta[15 i + 6 ..]  = v_i - v0_i                            3
 *   delta[15 i + 9 ..]  = b_i - b0_i                            6, (acc, gyro)
 *   error = c + g^T delta + 0.5 delta^T H delta
 * vus_navb_eval_step retracts velocities and biases by plain addition, so their differences are exact.  H [15 m, 15 m]
 * symmetric, row-major, both triangles stored; g the gradient at delta = 0; c a constant.  Linearised at the state the
 * factor contributes the blocks of H unchanged and the gradient g + H delta (the H = I choice of `window_prior`); at a node
 * step dp the linear error is error + (g + H delta)^T d + 0.5 d^T H d, d the 15 m step coordinates of the window.  There is
 * no robust model.  H need not be positive definite; vus_nav_window_prior_check refuses what vus_window_prior_check does.
 *
 * Nodes (pose_stride 3): row r of H belongs to keyframe first + r / 15 and, with q = r % 15, to
 *   q < 6: node 3 k, coordinate q;   q < 9: node 3 k + 1, coordinate q - 6;   else: node 3 k + 2, coordinate q - 9.
 * The three padding coordinates of a velocity node appear in neither H, g nor delta, and the family never reads or writes
 * them in Sband, gs or dp.
 *
 * The products H delta and H (delta + d) are summed in a fixed order (a workgroup per row and vector, each lane's columns
 * ascending, then its fixed LDS tree), the energies by the fixed-order reduce of the other families, the assembly by one
 * thread per target element without atomics: two runs give the same bits.
 */
#ifndef VUS_FIXED_LAG_NAV_H
#define VUS_FIXED_LAG_NAV_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_nav_window_prior {
  int n_poses;      /* keyframes of the problem (n_nodes = 3 n_poses) */
  int first;        /* first keyframe of the window */
  int m;            /* keyframes of the window: first .. first + m - 1 */
  const double* x0; /* [m, 12] linearisation poses, flat12 (row-major R, then t) */
  const double* v0; /* [m, 3] linearisation velocities */
  const double* b0; /* [m, 6] linearisation biases (acc, gyro) */
  const double* H;  /* [15 m, 15 m] row-major, symmetric, both triangles */
  const double* g;  /* [15 m] gradient at delta = 0 */
  double c;         /* the constant of the error */
} vus_nav_window_prior;

/* Host-side validation against a band of `band` NODES (reads H, g, x0, v0 and b0 back: one blocking copy each): m >= 1,
 * first >= 0, first + m <= n_poses, 3 m - 1 <= band, c finite, every entry of H, g, x0, v0 and b0 finite,
 * |H_ab - H_ba| <= 1e-12 of the largest |entry| of H (round-off), no negative diagonal entry.  The other entry points
 * check sizes and pointers only: call this once per prior. */
int vus_nav_window_prior_check(const vus_nav_window_prior* P, int band, void* stream);

/* doubles of `work` for the entry points below */
long long vus_nav_window_prior_work_doubles(const vus_nav_window_prior* P);

/* grad [15 m] = g + H delta at (poses [n_poses, 12], vels [n_poses, 3], biases [n_poses, 6]);  err[0] = the error there,
 * the linear error at a zero step. */
int vus_nav_window_prior_linearize(const vus_nav_window_prior* P, const double* poses, const double* vels, const double* biases,
                                   double* grad, double* err, double* work, void* stream);

/* Sband [3 n_poses, band + 1, 36] += the entries of H (lower block triangle; the padding coordinates of a velocity node are
 * left alone), gs [3 n_poses, 6] += grad on the window's coordinates.  One thread per target element, no atomics.  Call
 * after vus_ba_schur, before vus_navb_assemble. */
int vus_nav_window_prior_assemble(const vus_nav_window_prior* P, const double* grad, int band, double* Sband, double* gs,
                                  void* stream);

/* out[0] = error + (g + H delta)^T d + 0.5 d^T H d with d the window's coordinates of the node step dp [3 n_poses, 6]
 * (summed as c + g^T u + 0.5 u^T H u, u = delta + d);  out[1] = the error at (new_poses, new_vels, new_biases). */
int vus_nav_window_prior_eval_step(const vus_nav_window_prior* P, const double* poses, const double* vels, const double* biases,
                                   const double* dp, const double* new_poses, const double* new_vels, const double* new_biases,
                                   double* out, double* work, void* stream);

/* err[0] = the error at (poses, vels, biases): the factor's term of NonlinearFactorGraph.error(). */
int vus_nav_window_prior_error(const vus_nav_window_prior* P, const double* poses, const double* vels, const double* biases,
                               double* err, double* work, void* stream);

/* What vus_ba_band_marginalize leaves of a pose_stride 3 system on w whole keyframes, H18 [18 w, 18 w] and g18 [18 w] (18
 * coordinates per keyframe, those of the nodes X, V, B in turn), without the velocity padding: H15 [15 w, 15 w] and
 * g15 [15 w] in the order of vus_nav_window_prior.  The padding rows of a system assembled by vus_navb_assemble are an exact
 * unit diagonal with a zero gradient that no elimination step touches: they carry nothing.  1 <= w <= 1365. */
int vus_nav_window_prior_compact(const double* H18, const double* g18, int w, double* H15, double* g15, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_FIXED_LAG_NAV_H */
