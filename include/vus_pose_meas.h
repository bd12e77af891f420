/* vus_pose_meas.h -- partial absolute measurements on keyframe poses of the bundle adjustment (part of the C ABI of
 * include/vus.h, which includes this file; it can also be included on its own): a position fix (GPS at the surface, USBL /
 * LBL, a pressure sensor's depth as a position fix with two wide sigmas), optionally of a transponder mounted off the body
 * origin, and an attitude fix (AHRS, compass).  All pointers are device pointers, every call is asynchronous on `stream`,
 * allocates nothing and returns 0 or a negative VUS_E_* code, as in vus.h.
 *
 * Semantics (GTSAM 4.x GPSFactor, GPSFactorArm, PoseTranslationPrior<Pose3>, PoseRotationPrior<Pose3>; recalled, not
 * checked against an upstream build).  Pose X = (R, t) body-to-world, tangent order (omega, v), retract X Exp(xi) -- the
 * conventions of PriorFactorPose3 here.  Every factor is unary on one pose, has three residual rows and the diagonal
 * whitening W = diag(1 / sigma):
 *   VUS_POSE_MEAS_POSITION   r = W (t + R a - m)     m the measured world position, a the lever arm in the body frame
 *                            J = W [ -R [a]x , R ]   (3 x 6; the true derivative through the retraction)
 *   VUS_POSE_MEAS_ROTATION   r = W Log(Rm^T R)       Rm the measured rotation
 *                            J = W [ I3 , 0 ]        (the derivative of Log is not applied: gtsam's PoseRotationPrior, and the
 *                                                    H = I choice of the pose prior and the between factor here)
 * Each factor may carry its own robust model (include/vus_robust.h, Block reweighting), exactly as the between factors
 * do: with d = |r| its residual and Jacobian rows are scaled by sqrt(w(d)).  The linear slots hold
 * 0.5 sum w |b + J delta|^2, the nonlinear ones sum rho(d).  Several factors on one pose, of either kind, are summed.
 *
 * Where it enters: the factor touches its pose alone, so it adds to the pose's 6 x 6 information block Hpp and gradient gp
 * (gp = sum J^T r, the sign of the pose prior) after the observations were linearised and before the landmark Schur step.
 * The Schur step, the band solve, the back-substitution, the retraction and the marginals read Hpp and gp and never see the
 * factor itself; the node layout (pose_stride) matters to the step dp of vus_pose_meas_eval_step only.
 *
 * Assembly is deterministic: the factors are sorted by pose into a CSR (built once per graph on the host), one thread
 * owns one factor-carrying pose, sums its factors in CSR order in registers and adds the sums with plain loads and stores
 * (no atomics); the error sums are per-workgroup partials in a fixed tree order, summed in index order by one last pass.
 * Two runs give bit-identical Hpp, gp and scalars.
 *
 * These entry points have no `_cpu` twin in the oracle library: their CPU statement is the numpy reference of the test
 * suite (tests/pose_meas_ref.py). */
#ifndef VUS_POSE_MEAS_H
#define VUS_POSE_MEAS_H
#include "vus.h"
#include "vus_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_POSE_MEAS_POSITION 0
#define VUS_POSE_MEAS_ROTATION 1

typedef struct vus_pose_meas {
  int n;                   /* factors */
  int n_poses;             /* poses of the vus_ba_problem they belong to */
  int pose_stride;         /* 1, 2 or 3, as in vus_ba_problem: pose i is camera-side node pose_stride * i */
  int n_rows;              /* DISTINCT poses carrying at least one factor */
  const int* row_pose;     /* [n_rows] distinct poses carrying a factor, ascending */
  const int* row_ptr;      /* [n_rows+1] CSR into the arrays below (factors sorted by pose, graph order within a pose) */
  const int* kind;         /* [n] VUS_POSE_MEAS_POSITION / _ROTATION */
  const double* meas;      /* [n,9] POSITION: m(3), a(3), 0(3);  ROTATION: Rm row-major */
  const double* w;         /* [n,3] 1/sigma */
  const int* loss_kind;    /* [n] VUS_LOSS_* of each factor (VUS_LOSS_GAUSSIAN: no robust model) */
  const double* loss_k;    /* [n] its parameter, whitened units (ignored for VUS_LOSS_GAUSSIAN) */
} vus_pose_meas;

/* n == 0 (then n_rows == 0 and the arrays may be null) is valid for every call below: nothing is launched, the outputs
 * that are sums are set to 0, Hpp and gp are left as they are. */

/* Host-side validation of a factor set (reads the arrays back: one blocking copy per array).  row_pose strictly ascending
 * in [0, n_poses), row_ptr rising from 0 to n with no empty row, every kind known, every w finite and > 0, every
 * measurement finite, every Rm orthonormal within 1e-9 with det > 0, every loss kind known with a finite k > 0.  The other
 * entry points check sizes and pointers only: call this once per factor set. */
int vus_pose_meas_check(const vus_pose_meas* M, void* stream);

/* After any vus_ba_linearize* form and before vus_ba_schur, at the `poses` [n_poses, 12] that call linearised at: for
 * every pose i = row_pose[r], Hpp[i] (full 6 x 6, row-major) gains sum J^T J and gp[i] gains sum J^T r of its factors,
 * whitened and (robust-)weighted.  err[0] = 0.5 sum w d^2, the linear error at delta = 0, a slot of the caller's: it is
 * not added to the scalar of the observations.  work: vus_pose_meas_work_doubles(M) doubles. */
int vus_pose_meas_linearize(const vus_pose_meas* M, const double* poses, double* Hpp, double* gp, double* err,
                            double* work, void* stream);
long long vus_pose_meas_work_doubles(const vus_pose_meas* M);

/* out[0] = 0.5 sum w |b + J dp[pose_stride * i]|^2 with w, b, J at the OLD poses and dp [pose_stride * n_poses, 6] the
 * node step (only the pose nodes are read);  out[1] = the error (sum rho) at new_poses (from vus_ba_eval_step). */
int vus_pose_meas_eval_step(const vus_pose_meas* M, const double* poses, const double* dp, const double* new_poses,
                            double* out, double* work, void* stream);

/* err[0] = the error (sum rho) of the factors at poses: their term of NonlinearFactorGraph.error(). */
int vus_pose_meas_error(const vus_pose_meas* M, const double* poses, double* err, double* work, void* stream);

/* w_out [n] = the weight w(d) of every factor at poses, in CSR order (all ones for Gaussian factors). */
int vus_pose_meas_weights(const vus_pose_meas* M, const double* poses, double* w_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_POSE_MEAS_H */
