"""Numpy reference of PriorFactorPoint3 on observed landmarks (include/vus_point_prior.h) for the tests: mono_ref.MonoBA
with the prior term

    r = (p_j - mean) / sigma,   J = diag(1 / sigma),   error 0.5 |r|^2      (gtsam::PriorFactor<Point3>, never reweighted)

added to the per-landmark sums V / gl, to the error and to the step evaluation.  The damped solve, the LM and the dense
information matrix are inherited unchanged: they read V, gl and the error scalars only.  This file is the CPU statement of
the feature; it also draws the prior set and the problem of the GPU tests."""
import numpy as np

import mono_problem
import mono_ref

STEREO_LM, MONO_LM = mono_problem.STEREO_LM, mono_problem.MONO_LM
TRIPLE_LM, FAR_LM = 20, 30          # three priors on one landmark; a mean metres away from the landmark's value
AXIS_SIGMAS = (0.05, 0.7, 5.0)      # differs per axis: a mix-up of the xx / yy / zz slots 0 / 3 / 5 shows


class PointPriorBA(mono_ref.MonoBA):
    """MonoBA plus priors (idx [n], mean [n,3], sigmas [n,3]) on landmarks, in any order, several on one landmark summed."""

    def __init__(self, *args, point_priors=None, **kw):
        super().__init__(*args, **kw)
        idx, mean, sig = point_priors if point_priors is not None else (np.zeros(0, np.int64), np.zeros((0, 3)), np.ones((0, 3)))
        self.pp_idx = np.asarray(idx, np.int64).reshape(-1)
        self.pp_mean = np.asarray(mean, np.float64).reshape(-1, 3)
        self.pp_w = 1.0 / np.asarray(sig, np.float64).reshape(-1, 3)
        assert len(self.pp_idx) == len(self.pp_mean) == len(self.pp_w)

    # -- the prior term alone ----------------------------------------------------------------------
    def prior_residuals(self, points):
        """whitened residuals [n,3] of the priors at points [nL,3]"""
        return self.pp_w * (np.asarray(points, np.float64)[self.pp_idx] - self.pp_mean)

    def prior_error(self, points):
        return 0.5 * float(np.sum(self.prior_residuals(points) ** 2))

    def prior_error_of(self, j, p):
        """the error of the priors on landmark j with the landmark at p [3]"""
        sel = self.pp_idx == j
        return 0.5 * float(np.sum((self.pp_w[sel] * (np.asarray(p, np.float64) - self.pp_mean[sel])) ** 2))

    def prior_blocks(self, points):
        """(V [nL,6] upper triangle xx,xy,xz,yy,yz,zz, gl [nL,3]): J^T J and J^T r of the priors summed per landmark"""
        V, gl = np.zeros((self.nL, 6)), np.zeros((self.nL, 3))
        w2 = self.pp_w ** 2
        for k, slot in enumerate((0, 3, 5)):
            np.add.at(V[:, slot], self.pp_idx, w2[:, k])
        np.add.at(gl, self.pp_idx, self.pp_w * self.prior_residuals(points))
        return V, gl

    # -- MonoBA with the term in place -------------------------------------------------------------
    def error(self, poses, points):
        return super().error(poses, points) + self.prior_error(points)

    def linearize(self, poses, points):
        """as MonoBA's, with the priors in V, gl and err; `obs_err` / `pp_err` keep the two scalars apart"""
        lin = super().linearize(poses, points)
        V, gl = self.prior_blocks(points)
        self._pp_points = np.array(points, np.float64)
        lin["V"] = lin["V"] + V
        lin["gl"] = lin["gl"] + gl
        lin["obs_err"], lin["pp_err"] = lin["err"], self.prior_error(points)
        lin["err"] = lin["obs_err"] + lin["pp_err"]
        return lin

    def linear_error(self, dp, dl):
        return super().linear_error(dp, dl) + self.prior_error(self._pp_points + dl)

    def observation_errors(self, poses, points, dp, dl):
        """(linear error at the step, error at the new values) of the observations and pose priors alone, after
        linearize(): what the observation kernels report next to the prior's own scalars"""
        npo, npt = self.retract(poses, points, dp, dl)
        return super().linear_error(dp, dl), super().error(npo, npt)


# -- the problem and the prior set of the GPU tests ------------------------------------------------
def single_sighting(seq, lo=12):
    """seq with one landmark reduced to a single monocular sighting: the first landmark >= lo, other than the named ones,
    that has a mono row keeps its first mono row and loses the others.  Returns (seq, that landmark)."""
    named = {0, 5, STEREO_LM, MONO_LM, TRIPLE_LM, FAR_LM, len(seq["points_gt"]) - 1}
    ol, mono = seq["obs_point"], seq["mono"]
    lm = next(j for j in range(lo, len(seq["points_gt"])) if j not in named and mono[ol == j].any())
    keep = np.ones(len(ol), bool)
    keep[ol == lm] = False
    keep[np.nonzero((ol == lm) & mono)[0][0]] = True
    out = dict(seq)
    for key in ("obs_pose", "obs_point", "meas", "mono"):
        out[key] = seq[key][keep]
    assert (out["obs_point"] == lm).sum() == 1 and out["mono"][out["obs_point"] == lm].all()
    return out, lm


def prior_set(seq, single_lm):
    """(idx, mean, sigmas) in graph order -- deliberately not sorted by landmark: priors on landmark 0 and on the last
    one, three with different means and sigmas on TRIPLE_LM (not adjacent in the list), per-axis sigmas, a mean metres
    away on FAR_LM, the landmark with a single mono sighting, and STEREO_LM (which the stage tests put behind its
    cameras)."""
    gt, nL = seq["points_gt"], len(seq["points_gt"])
    rows = [(nL - 1, gt[nL - 1] + (0.02, -0.1, 0.3), AXIS_SIGMAS),
            (TRIPLE_LM, gt[TRIPLE_LM] + (0.1, 0.0, -0.2), (0.3, 0.3, 0.3)),
            (0, gt[0] + (-0.3, 0.01, 0.05), (5.0, 0.05, 0.7)),
            (single_lm, gt[single_lm] + (0.02, -0.01, 0.03), (0.2, 0.2, 0.2)),
            (TRIPLE_LM, gt[TRIPLE_LM] + (-0.05, 0.2, 0.1), (0.7, 5.0, 0.05)),
            (STEREO_LM, gt[STEREO_LM] + (0.0, 0.05, -0.05), (0.1, 0.1, 0.1)),
            (FAR_LM, gt[FAR_LM] + (4.0, -3.0, 5.0), (2.0, 5.0, 0.7)),
            (TRIPLE_LM, gt[TRIPLE_LM] + (0.0, -0.1, 0.0), (1.0, 0.4, 2.0))]
    idx = np.array([r[0] for r in rows], np.int64)
    return idx, np.array([r[1] for r in rows], np.float64), np.array([r[2] for r in rows], np.float64)
