/* vus_fixed_lag.h -- fixed-lag smoothing on the GPU (part of the C ABI of include/vus.h, which includes this file; it can
 * also be included on its own): a dense Gaussian prior over a window of consecutive keyframe poses (the add-on family
 * `window_prior`), and the kernel that forms such a prior by marginalising the head of the reduced camera system.
 * All pointers are device pointers, every call is asynchronous on `stream`, allocates nothing and returns 0 or a negative
 * VUS_E_* code, as in vus.h.  Every argument is checked on the host before anything is launched.
 *
 * Semantics (GTSAM's LinearContainerFactor holding a HessianFactor, recalled, not checked against an upstream build): for
 * the poses first .. first + m - 1 with linearisation poses x0 [m, 12] (flat12),
 *   delta_i = Local(x0_i, x_i) = Log(x0_i^-1 x_i)  (tangent order (omega, v)),  delta = their stack, 6 m values
 *   error(x) = c + g^T delta + 0.5 delta^T H delta
 * H [6 m, 6 m] symmetric, row-major, both triangles stored; g the gradient at delta = 0; c a constant.  Linearised at x the
 * factor contributes the blocks of H unchanged and the gradient g + H delta; the linear system's error at a zero step is
 * error(x).  The derivative of Local is not applied -- the H = I choice of the prior and between factors here.  At a step
 * dp the linear error is error(x) + (g + H delta)^T dp + 0.5 dp^T H dp.  There is no robust model.
 * H need not be positive definite: the marginal of a graph without an absolute reference is positive semi-definite, its
 * gauge directions free.  vus_window_prior_check refuses a non-finite entry, an asymmetry beyond round-off and a negative
 * diagonal entry.
 *
 * Nodes: the family serves the pose-only layout (pose_stride 1): pose p is node p.
 *
 * The products H delta and H dp are summed in a fixed order (a workgroup per row, its fixed LDS tree), the energies by
 * the fixed-order reduce of the other families, the assembly by one thread per target element without atomics: two runs
 * give the same bits.
 */
#ifndef VUS_FIXED_LAG_H
#define VUS_FIXED_LAG_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_window_prior {
  int n_poses;      /* poses (= camera-side nodes) of the problem */
  int first;        /* first pose of the window */
  int m;            /* poses of the window: first .. first + m - 1 */
  const double* x0; /* [m, 12] linearisation poses, flat12 (row-major R, then t) */
  const double* H;  /* [6 m, 6 m] row-major, symmetric, both triangles */
  const double* g;  /* [6 m] gradient at delta = 0 */
  double c;         /* the constant of error(x) */
} vus_window_prior;

/* Host-side validation against a band of `band` nodes (reads H, g and x0 back: one blocking copy each): m >= 1,
 * first >= 0, first + m <= n_poses, m - 1 <= band, c finite, every entry of H, g and x0 finite, |H_ab - H_ba| <= 1e-12 of
 * the largest |entry| of H (round-off), no negative diagonal entry.  The other entry points check sizes and
 * pointers only: call this once per prior. */
int vus_window_prior_check(const vus_window_prior* P, int band, void* stream);

/* doubles of `work` for the entry points below */
long long vus_window_prior_work_doubles(const vus_window_prior* P);

/* grad [6 m] = g + H delta at `poses` [n_poses, 12];  err[0] = error(poses), the linear error at a zero step. */
int vus_window_prior_linearize(const vus_window_prior* P, const double* poses, double* grad, double* err, double* work,
                               void* stream);

/* Sband [n_poses, band + 1, 36]: block (first + a, a - b) += H_ab for a >= b;  gs [n_poses, 6]: rows of the window += grad.
 * One thread per target element, no atomics.  Call where vus_between_assemble stands: after vus_ba_schur. */
int vus_window_prior_assemble(const vus_window_prior* P, const double* grad, int band, double* Sband, double* gs, void* stream);

/* out[0] = error(poses) + (g + H delta)^T d + 0.5 d^T H d with d the rows of the window of the node step dp [n_poses, 6]
 * (summed as c + g^T u + 0.5 u^T H u, u = delta + d);  out[1] = error(new_poses). */
int vus_window_prior_eval_step(const vus_window_prior* P, const double* poses, const double* dp, const double* new_poses,
                               double* out, double* work, void* stream);

/* err[0] = error(poses): the factor's term of NonlinearFactorGraph.error(). */
int vus_window_prior_error(const vus_window_prior* P, const double* poses, double* err, double* work, void* stream);

/* ---- marginalising the head of the reduced camera system ---------------------------------------------------------------
 * Sband [n_nodes, band + 1, 36] (entry (i, s) = block (i, i - s), row-major) and gs [n_nodes, 6]: the UNDAMPED, UNFACTORISED
 * system vus_ba_schur(lambda = 0) and the assemble stages leave.  Neither is modified.  With M = nodes 0 .. n_drop - 1 and
 * R = the rest (w = n_nodes - n_drop of them):
 *   H [6 w, 6 w] = S_RR - S_RM S_MM^-1 S_MR   (row-major, both triangles)
 *   g [6 w]      = g_R - S_RM S_MM^-1 g_M
 *   quad[0]      = g_M^T S_MM^-1 g_M
 * Requires 1 <= n_drop < n_nodes and n_nodes - n_drop <= band + 1, so that every block of S_RR is a stored one, and
 * 0 <= band < n_nodes <= 4096 (a band wider than the matrix stores nothing more).
 * status[0] = 0, or 1 + row of the first non-positive pivot of S_MM (the band solve's convention); the outputs are then
 * meaningless.
 * The system and its gradient (one more row) are copied to a dense lower triangle in `work`; per 8-node (48-row) panel of
 * M three launches -- the 48 x 48 factor in one workgroup, the triangular solve of the rows below, the outer product
 * subtracted from the trailing part on v_mfma_f64_16x16x4_f64 -- and one that writes H, g and quad.  No workgroup waits for
 * another; fixed summation order: two calls give the same bits.
 * work: vus_ba_band_marginalize_work_doubles(n_nodes, band, n_drop) doubles (0 for invalid sizes). */
long long vus_ba_band_marginalize_work_doubles(int n_nodes, int band, int n_drop);
int vus_ba_band_marginalize(const double* Sband, int n_nodes, int band, const double* gs, int n_drop, double* H, double* g,
                            double* quad, int* status, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_FIXED_LAG_H */
