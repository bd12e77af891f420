/* vus_between.h -- BetweenFactor<Pose3> on the GPU (part of the C ABI of include/vus.h, which includes this file; it can
 * also be included on its own): odometry and loop-closure constraints between two keyframe poses, added to the reduced
 * camera system after the landmark Schur step.  All pointers are device pointers, every call is asynchronous on
 * `stream`, allocates nothing and returns 0 or a negative VUS_E_* code, as in vus.h.
 *
 * Semantics (GTSAM 4.x default build, recalled, not checked against an upstream build): tangent order (omega, v),
 * retract T Exp(xi), Local(T, T2) = Log(T^-1 T2) -- the conventions of PriorFactorPose3 here.
 *   hx = T1^-1 T2,   r = Log(measured^-1 hx),   error = 0.5 |W r|^2   (W = diag(1/sigma))
 *   H1 = -Ad(hx^-1),  H2 = I6   (the Jacobians of Pose3::between; the derivative of Local is not applied -- GTSAM
 *   without SLOW_BUT_CORRECT_BETWEENFACTOR, and the H = I choice of the prior factor here)
 * Each factor may carry its own robust model (include/vus_robust.h, Block reweighting; Gaussian odometry next to robust
 * loop closures): its whitened residual and Jacobian rows are scaled by sqrt(w(|W r|)).  The linear slots hold
 * 0.5 sum w |b + J delta|^2, the nonlinear ones sum rho(|W r|).
 * Full-covariance models (noiseModel.Gaussian): with `sqrt_info` set, W of factor f is its upper-triangular R, R^T R = cov^-1,
 * in place of diag(1/sigma) in every formula above -- whitened residual R r, whitened Jacobians R H1 and R, d = |R r| for
 * the robust weight, which stays one weight per factor (Block).  Every factor of such a set uses its R (a diagonal factor
 * carries R = diag(1/sigma)) and `w` is not read.  J2^T J2 = w R^T R is then a full block.  Any R with R^T R = cov^-1 gives
 * the same error and the same products up to round-off; the kernels sum over the residual rows in ascending order.
 *
 * Nodes: endpoint node = pose_stride * pose (pose_stride 1, 2 or 3 as in vus_ba_problem), so one set of kernels serves
 * every node layout.  Either key order is allowed, several factors on one pair are summed, node1 == node2 is invalid.
 *
 * Assembly is deterministic: a CSR built once per graph on the host lists, for every 6 x 6 target block (node, s) of the
 * band that between factors touch, the factor terms that land in it, in a fixed order.  A term is 4 f + kind:
 *   kind 0  J1^T J1 of factor f     (node1, 0)       its gradient J1^T r goes to node1
 *   kind 1  J2^T J2                  (node2, 0)       J2^T r to node2
 *   kind 2  J1^T J2                  (node1, node1 - node2), node1 > node2
 *   kind 3  (J1^T J2)^T = J2^T J1    (node2, node2 - node1), node2 > node1
 * Each target element is summed by one thread over its list: two runs give bit-identical Sband / gs.
 */
#ifndef VUS_BETWEEN_H
#define VUS_BETWEEN_H
#include "vus.h"
#include "vus_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_between_factors {
  int n;                      /* factor count */
  int n_nodes;                /* camera-side nodes of the problem (pose_stride * n_poses) */
  int pose_stride;            /* 1, 2 or 3: pose = node / pose_stride */
  const int* node1;           /* [n] pose_stride * pose of key1 */
  const int* node2;           /* [n] pose_stride * pose of key2 */
  const double* meas;         /* [n, 12] measured T1^-1 T2, flat12 (row-major R, then t) */
  const double* w;            /* [n, 6] whitening weights 1/sigma, tangent order (omega, v) */
  const int* loss_kind;       /* [n] VUS_LOSS_* of each factor (VUS_LOSS_GAUSSIAN: no robust model) */
  const double* loss_k;       /* [n] its parameter, whitened units (ignored for VUS_LOSS_GAUSSIAN) */
  int n_targets;              /* target blocks */
  const int* tgt_node;        /* [n_targets] row node of the block */
  const int* tgt_s;           /* [n_targets] block diagonal s: the block is (node, node - s) */
  const int* tgt_ptr;         /* [n_targets + 1] CSR row pointers into tgt_terms */
  const int* tgt_terms;       /* [tgt_ptr[n_targets]] 4 f + kind, in summation order */
  const double* sqrt_info;    /* NULL: the diagonal model of `w`, exactly as before the field existed.  Else [n, 36] row-major:
                                 per factor the upper-triangular R with R^T R = cov^-1 (positive diagonal); whitened
                                 residual R r, whitened Jacobians R H1 and R.  The kernels read the 21 entries on and above
                                 the diagonal only; `w` is then not read (and may be NULL).  Appended last: a caller that
                                 fills the fields before it and zero-initialises the struct keeps the diagonal model. */
} vus_between_factors;

/* Host-side validation of a factor set against a band of `band` nodes (reads the index arrays back: one blocking copy per
 * array).  Every node in [0, n_nodes), node1 != node2, |node1 - node2| <= band, every loss kind known with a finite
 * k > 0, every target inside the band with its terms in range and of the right block; with `sqrt_info`, every entry on or
 * above the diagonal finite and every diagonal entry > 0 (the factor's number is in the message).  The other entry points
 * check sizes and pointers only: call this once per factor set. */
int vus_between_check(const vus_between_factors* B, int band, void* stream);

/* Per factor at `poses` [n_poses, 12], whitened and (robust-)weighted:  lin [n, 120] = J1^T J1 (36), J1^T J2 (36, row-major,
 * rows of node1), J2^T J2 (36: diagonal under a diagonal model, full under sqrt_info), J1^T r (6), J2^T r (6);  err[0] =
 * 0.5 sum w |b|^2, the linear error at delta = 0.
 * work: vus_between_work_doubles(B) doubles. */
int vus_between_linearize(const vus_between_factors* B, const double* poses, double* lin, double* err, double* work,
                          void* stream);
long long vus_between_work_doubles(const vus_between_factors* B);

/* Sband [n_nodes, band + 1, 36] += the between blocks, gs [n_nodes, 6] += the between gradient (no atomics, fixed order).
 * Call after vus_ba_schur (which writes Sband / gs and damps the pose blocks) and before vus_nav_assemble /
 * vus_navb_assemble where there is one (vus_nav_assemble copies -gs into its right-hand side). */
int vus_between_assemble(const vus_between_factors* B, const double* lin, int band, double* Sband, double* gs, void* stream);

/* out[0] = 0.5 sum w |b + J1 d1 + J2 d2|^2 with w, b, J at the OLD poses and d the node step dp [n_nodes, 6];
 * out[1] = the error (sum rho) at new_poses (from vus_ba_eval_step). */
int vus_between_eval_step(const vus_between_factors* B, const double* poses, const double* dp, const double* new_poses,
                          double* out, double* work, void* stream);

/* err[0] = the error (sum rho) of the between factors at poses: their term of NonlinearFactorGraph.error(). */
int vus_between_error(const vus_between_factors* B, const double* poses, double* err, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_BETWEEN_H */
