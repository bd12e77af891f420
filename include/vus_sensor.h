/* vus_sensor.h -- stereo factors with a camera-to-body extrinsic (part of the C ABI of include/vus.h, which includes
 * this file; it can also be included on its own).
 *
 * gtsam::GenericStereoFactor<Pose3, Point3>(measured, model, poseKey, landmarkKey, K, body_P_sensor): the pose variable
 * X(i) is the vehicle body (the frame of the ImuFactor and of the DVL velocity), and the left camera sits at
 *
 *   C = X o S,   S = body_P_sensor = (Rs, ts),   X = (Rb, tb):   C = (Rb Rs, tb + Rb ts)
 *
 * One extrinsic per graph, like the one noise model and the one Cal3_S2Stereo.  The residual, the cheirality test
 * (z <= 0 in the CAMERA frame: residual 2 fx / sigma, zero Jacobians) and the landmark Jacobian H2 are those of the
 * plain stereo factor evaluated at C.  A step of the body, X Exp(xi) S = C Exp(Ad(S^-1) xi), moves the camera by the
 * adjoint of S^-1, so with the tangent ordered [omega, v] as everywhere in this library
 *
 *   H1_body = H1_cam Ad(S^-1),   Ad(S^-1) = [ Rs^T            0    ]
 *                                           [ -Rs^T [ts]x     Rs^T ]
 *
 * and W = H1_body^T H2, Hpp = sum H1_body^T H1_body = Ad^T (sum H1_cam^T H1_cam) Ad, gp = Ad^T (sum H1_cam^T r).
 * Every later stage (vus_ba_schur, the band solve, vus_ba_backsub, the retraction, the marginals) consumes W, V, gl,
 * Hpp, gp and a BODY-tangent step dp and is unchanged; priors, between factors and the inertial factors act on X as
 * before.
 *
 * The entry points below take the arguments of vus_ba_linearize / vus_ba_eval_step / vus_ba_error /
 * vus_ba_stereo_weights and follow their contract (same buffers, same slots: err[0], out[0] = linear error at the step,
 * out[1] = nonlinear error at the new values), with two trailing arguments:
 *   loss     the robust model of include/vus_robust.h; NULL = Gaussian.  One set of entry points serves both: under a
 *            robust model the slots hold what the `_robust` twins report (0.5 sum w d^2 in the linear slots, sum rho in
 *            the nonlinear ones), and the factor's scalar sqrt(w) scales r, H1_body and H2 alike.
 *   sensor   the extrinsic; must not be NULL.  Validated on the host before any launch: 12 finite values and
 *            max |Rs^T Rs - I| <= 1e-9.
 * The identity extrinsic computes what the entry points without `_sensor` compute (to rounding; they stay the ones to
 * call without an extrinsic, and launch the same kernels as before).
 *
 * These entry points have no `_cpu` twin in the oracle library: their CPU statement is the numpy reference of the test
 * suite, which composes C in float64, calls the oracle's stereo factor there and multiplies H1 by Ad(S^-1). */
#ifndef VUS_SENSOR_H
#define VUS_SENSOR_H
#include "vus.h"
#include "vus_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_ba_sensor {
  double T[12];     /* body_P_sensor in the pose layout used everywhere: R row-major (9), then t (3) */
} vus_ba_sensor;

int vus_ba_linearize_sensor(const vus_ba_problem* P, const double* poses, const double* points, double* W, double* V,
                            double* gl, double* Hpp, double* gp, double* err, double* work, void* stream,
                            const vus_ba_loss* loss, const vus_ba_sensor* sensor);
int vus_ba_eval_step_sensor(const vus_ba_problem* P, const double* poses, const double* points, const double* dp,
                            const double* dl, double* new_poses, double* new_points, double* out, double* work,
                            void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor);
int vus_ba_error_sensor(const vus_ba_problem* P, const double* poses, const double* points, double* err, double* work,
                        void* stream, const vus_ba_loss* loss, const vus_ba_sensor* sensor);
/* vus_ba_stereo_weights with the camera at X o S; loss = NULL gives all ones */
int vus_ba_stereo_weights_sensor(const vus_ba_problem* P, const vus_ba_loss* loss, const double* poses,
                                 const double* points, double* w, void* stream, const vus_ba_sensor* sensor);

#ifdef __cplusplus
}
#endif
#endif /* VUS_SENSOR_H */
