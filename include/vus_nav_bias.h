/* vus_nav_bias.h -- inertial graphs with ONE IMU BIAS PER KEYFRAME (part of the C ABI of include/vus.h, which includes this
 * file; it can also be included on its own).  GTSAM's usual visual-inertial graph (ImuFactorsExample):
 *   ImuFactor(X(i), V(i), X(i+1), V(i+1), B(i), pim)        each ImuFactor at the bias of its EARLIER keyframe
 *   BetweenFactorConstantBias(B(i), B(i+1), m, sigma)       e = (b_j - b_i) - m, Jacobians -I and +I (vector space)
 *   PriorFactorConstantBias(B(k), mu, sigma)                e = b - mu
 * next to the DVL factors and velocity priors of vus_nav_factors.  All pointers are device pointers, every call is
 * asynchronous on `stream`, allocates nothing and returns 0 or a negative VUS_E_* code, as in vus.h.  The arguments are
 * checked on the host before anything is launched; the index arrays are read back for that (a few kB, one blocking copy
 * per array and call).
 *
 * Node layout (vus_ba_problem.pose_stride = 3): node 3i = X(i), node 3i+1 = V(i) padded to 6 (dims 3..5 inert: unit
 * diagonal, zero right-hand side), node 3i+2 = B(i) (acc, gyro).  There is no border: every variable is a band node.
 * An ImuFactor couples nodes 3i .. 3i+4 (4 apart), a bias between-factor nodes 3i+2 and 3i+5 (3 apart), so the inertial
 * blocks fill the 5 innermost block diagonals and the node band is at least 4.
 */
#ifndef VUS_NAV_BIAS_H
#define VUS_NAV_BIAS_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_navb_factors {
  int n_imu;
  const int* imu_i;          /* [n_imu] pose index of the earlier state; the factor uses bias B(imu_i) */
  const int* imu_j;          /* [n_imu] = imu_i + 1 */
  const double* imu_pim;     /* [n_imu,148] as vus_nav_factors */
  const double* imu_W;       /* [n_imu,81] */
  double gravity[3];
  int n_dvl;
  const int* dvl_pose;       /* [n_dvl] */
  const double* dvl_meas;    /* [n_dvl,3] body-frame velocity */
  const double* dvl_w;       /* [n_dvl] 1/sigma */
  int n_vprior;
  const int* vprior_idx;     /* [n_vprior] */
  const double* vprior_v;    /* [n_vprior,3] */
  const double* vprior_w;    /* [n_vprior,3] 1/sigma */
  int n_bbetween;
  const int* bb_i;           /* [n_bbetween] earlier bias index */
  const int* bb_j;           /* [n_bbetween] = bb_i + 1 */
  const double* bb_meas;     /* [n_bbetween,6] measured b_j - b_i (acc, gyro) */
  const double* bb_w;        /* [n_bbetween,6] 1/sigma (diagonal model) */
  int n_bprior;
  const int* bp_idx;         /* [n_bprior] bias index */
  const double* bp_mean;     /* [n_bprior,6] */
  const double* bp_w;        /* [n_bprior,6] 1/sigma */
} vus_navb_factors;

/* Residuals and Jacobians of every inertial factor at (poses [n_poses,12], vels [n_poses,3], biases [n_poses,6]),
 * accumulated into
 *   Snav [3 n_poses, 5, 36]  blocks (node, node - s), s = 0..4   (undamped)
 *   gnav [6 * 3 n_poses]     node gradient
 *   err  [1]                 0.5 * sum |whitened residual|^2 of these factors
 * Every block gets its addends with f64 atomics (a bias block up to two IMU factors, two between-factors and priors), so
 * two runs agree to ~1e-16 relative, not bitwise.  work: vus_navb_work_doubles(N) doubles. */
int vus_navb_linearize(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                       const double* biases, double* Snav, double* gnav, double* err, double* work, void* stream);
long long vus_navb_work_doubles(const vus_navb_factors* N);

/* Per lambda, after vus_ba_schur (pose_stride 3): Sband += Snav on the 5 innermost block diagonals; velocity nodes get
 * lambda on their 3 real coordinates and 1 on the 3 padding coordinates, bias nodes lambda on all 6; gs += gnav.
 * n_nodes = 3 n_poses, band >= min(4, n_nodes - 1).  The step is then ONE single-right-hand-side band solve. */
int vus_navb_assemble(int n_nodes, int band, double lambda, const double* Snav, const double* gnav, double* Sband,
                      double* gs, void* stream);

/* new_vels = vels + dv, new_biases = biases + db (both from the node step dc [6 * 3 n_poses]); out[0] = linearised
 * error of the inertial factors at the step (Jacobians at the OLD values), out[1] = their error at the new values
 * (new_poses from vus_ba_eval_step). */
int vus_navb_eval_step(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                       const double* biases, const double* dc, const double* new_poses, double* new_vels,
                       double* new_biases, double* out, double* work, void* stream);

/* err[0] = error of the inertial factors at (poses, vels, biases). */
int vus_navb_error(const vus_navb_factors* N, int n_poses, const double* poses, const double* vels,
                   const double* biases, double* err, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_NAV_BIAS_H */
