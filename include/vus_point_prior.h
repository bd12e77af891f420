/* vus_point_prior.h -- PriorFactor<Point3> on landmarks of the bundle adjustment (part of the C ABI of include/vus.h,
 * which includes this file; it can also be included on its own): a diagonal Gaussian prior on a landmark that stereo or
 * monocular factors observe -- a surveyed marker, a known dock, a sonar fix on a feature, or the landmark that fixes the
 * scale of a monocular graph.  All pointers are device pointers, every call is asynchronous on `stream`, allocates
 * nothing and returns 0 or a negative VUS_E_* code, as in vus.h.
 *
 * Semantics (gtsam::PriorFactor<Point3>): r = (p - mean) / sigma per axis, Jacobian diag(1 / sigma), error 0.5 |r|^2.
 * Diagonal, Isotropic and Unit models; no robust model (the factor is never reweighted, whatever model the observations
 * carry).  Several priors on one landmark are summed.
 *
 * Where it enters: the factor touches its landmark alone, so it adds to the landmark's 3 x 3 information block V and
 * gradient gl after the observations were linearised and before the landmark Schur step.  The Schur step, the band solve,
 * the back-substitution, the retraction and the marginals read V and gl and never see the factor itself.
 *
 * Assembly is deterministic: the factors are sorted by landmark into a CSR (built once per graph on the host), one thread
 * owns one prior-carrying landmark and adds its priors in CSR order with plain loads and stores; the error sums are
 * per-workgroup partials in a fixed tree order, summed in index order by one last pass.  Two runs give bit-identical
 * V, gl and scalars.
 */
#ifndef VUS_POINT_PRIOR_H
#define VUS_POINT_PRIOR_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vus_point_priors {
  int n;                  /* prior factors */
  int n_points;           /* landmarks of the vus_ba_problem they belong to */
  int n_rows;             /* DISTINCT landmarks carrying at least one prior */
  const int* row_point;   /* [n_rows] landmark index, ascending, distinct */
  const int* row_ptr;     /* [n_rows+1] CSR into mean / w (factors sorted by landmark, graph order within one) */
  const double* mean;     /* [n,3] */
  const double* w;        /* [n,3] 1/sigma */
} vus_point_priors;

/* n == 0 (then n_rows == 0 and the arrays may be null) is valid for every call below: nothing is launched, the outputs
 * that are sums are set to 0, V and gl are left as they are. */

/* Host-side validation of a factor set (reads the arrays back: one blocking copy per array).  row_point strictly
 * ascending in [0, n_points), row_ptr rising from 0 to n with no empty row, every w finite and > 0, every mean finite.
 * The other entry points check sizes and pointers only: call this once per factor set. */
int vus_point_prior_check(const vus_point_priors* Q, void* stream);

/* After any vus_ba_linearize* form and before vus_ba_schur, at the `points` [n_points, 3] that call linearised at:
 * for every landmark j = row_point[r], V[j] (upper triangle xx, xy, xz, yy, yz, zz) gains sum w^2 of each axis in its
 * slots 0, 3 and 5, and gl[j] gains sum w^2 (p_j - mean).  err[0] = 0.5 sum |w (p - mean)|^2, a slot of the caller's: it
 * is not added to the scalar of the observations.  work: vus_point_prior_work_doubles(Q) doubles. */
int vus_point_prior_linearize(const vus_point_priors* Q, const double* points, double* V, double* gl, double* err,
                              double* work, void* stream);
long long vus_point_prior_work_doubles(const vus_point_priors* Q);

/* out[0] = 0.5 sum |w (p + dl - mean)|^2 with dl [n_points, 3] the landmark step: the linearised error at the step,
 * exact because the factor is linear;  out[1] = the same from new_points (as vus_ba_eval_step wrote them), which differs
 * from out[0] by round-off only. */
int vus_point_prior_eval_step(const vus_point_priors* Q, const double* points, const double* dl, const double* new_points,
                              double* out, double* work, void* stream);

/* err[0] = 0.5 sum |w (p - mean)|^2 at points: the priors' term of NonlinearFactorGraph.error(). */
int vus_point_prior_error(const vus_point_priors* Q, const double* points, double* err, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_POINT_PRIOR_H */
