"""Host side of the stereo bundle adjustment: device-resident problem, workspace, and the
Levenberg-Marquardt control loop that drives the HIP kernels of csrc/ba.hip through the C ABI.

Mirrors what `gtsam.LevenbergMarquardtOptimizer(graph, initial, params).optimize()` does at
/root/reference/batch.py:337 (GTSAM's iterate / tryLambda / checkConvergence logic with the default
LevenbergMarquardtParams), for graphs of GenericStereoFactor3D + PriorFactorPose3 factors.  All
arithmetic (residuals, Jacobians, Schur complement, band Cholesky, retraction, errors) runs on the
GPU; this file only sequences launches and reads back three scalars per lambda trial.
"""
import ctypes
import math
import time
from ctypes import c_double
from collections import namedtuple
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _abi, _lib, ba_pack


# the structs the entry points take by address: their layouts are the headers' (include/vus.h and the vus_*.h next to it)
_CProblem = _abi.struct("vus_ba_problem")
_CTiles = _abi.struct("vus_ba_tiles")
_CLoss = _abi.struct("vus_ba_loss")
_CSensor = _abi.struct("vus_ba_sensor")
_CMono = _abi.struct("vus_ba_mono")
_CBetween = _abi.struct("vus_between_factors")
_CPointPriors = _abi.struct("vus_point_priors")
_CPoseMeas = _abi.struct("vus_pose_meas")
_CWindowPrior = _abi.struct("vus_window_prior")
_CNavWindowPrior = _abi.struct("vus_nav_window_prior")
_CNav = _abi.struct("vus_nav_factors")
_CNavBias = _abi.struct("vus_navb_factors")         # the fields of vus_nav_factors, then the bias factors
_CCombinedImu = _abi.struct("vus_cimu_factors")

# VUS_LOSS_* of include/vus_robust.h: robust noise models of the stereo factors (GTSAM mEstimator, Block reweighting)
LOSS_KINDS = {k: _abi.const("VUS_LOSS_" + k.upper())
              for k in ("gaussian", "huber", "cauchy", "tukey", "geman_mcclure", "welsch")}


def robust_loss(loss):
    """None, a kind name / VUS_LOSS_* number with its parameter `(kind, k)`, or an object with `.kind` and `.k`
    (gtsam.noiseModel.mEstimator.*) -> (kind number, k); (0, 0.0) is the plain Gaussian model."""
    if loss is None:
        return 0, 0.0
    kind, k = (loss.kind, loss.k) if hasattr(loss, "kind") else loss
    if isinstance(kind, str):
        if kind.lower() not in LOSS_KINDS:
            raise ValueError(f"unknown robust loss {kind!r} (one of {', '.join(LOSS_KINDS)})")
        kind = LOSS_KINDS[kind.lower()]
    kind, k = int(kind), float(k)
    if not 0 <= kind <= 5:
        raise ValueError(f"unknown robust loss kind {kind}")
    if kind == 0:
        return 0, 0.0
    if not (math.isfinite(k) and k > 0.0):
        raise ValueError(f"robust loss parameter k={k} must be finite and > 0")
    return kind, k


def sensor_flat12(body_P_sensor):
    """None, a 12-vector (R row-major, then t), a 4 x 4 matrix or an object with `.flat12()` (gtsam.Pose3) -> the 12
    float64 values of include/vus_sensor.h, or None.  The library validates them (finite, orthonormal rotation)."""
    if body_P_sensor is None:
        return None
    if hasattr(body_P_sensor, "flat12"):
        return np.array(body_P_sensor.flat12(), dtype=np.float64).reshape(12)
    a = body_P_sensor.detach().cpu().numpy() if torch.is_tensor(body_P_sensor) else np.asarray(body_P_sensor)
    a = np.array(a, dtype=np.float64)
    if a.shape == (4, 4):
        if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("body_P_sensor: the last row of a 4 x 4 pose matrix must be 0 0 0 1")
        return np.concatenate([a[:3, :3].reshape(9), a[:3, 3]])
    if a.size == 12 and a.ndim == 1:
        return a.copy()
    raise ValueError(f"body_P_sensor: a 12-vector, a 4 x 4 matrix or a Pose3 is expected, not an array of shape {a.shape}")


def _upload(a, device, dtype, shape=None):
    """A host array (numpy, list or tensor) as a contiguous device tensor of `dtype`, reshaped to `shape` if given."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)             # torch refuses negative strides
    t = torch.as_tensor(a).to(device=device, dtype=dtype)
    return (t if shape is None else t.reshape(shape)).contiguous()


def csr_rows(idx):
    """The CSR of include/vus_point_prior.h and include/vus_pose_meas.h on the host: (order, row_item, row_ptr) -- `order`
    sorts the factors stably by their item `idx` (a landmark or a pose; graph order within one item), row_item lists the
    distinct items ascending, row_ptr [n_rows + 1] points into the sorted factors."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    order = np.argsort(idx, kind="stable")
    row_item, first = np.unique(idx[order], return_index=True)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return order, i32(row_item), i32(np.append(first, len(idx)))


def _factor_losses(loss, n, what):
    """The robust models of the n factors of a set (`what` names it): `loss` is one model for all of them (robust_loss():
    None = Gaussian) or a list (not a tuple) of n, one per factor -> [(kind, k)] of length n."""
    if isinstance(loss, list) and len(loss) != n:
        raise ValueError(f"{what}: {len(loss)} robust models for {n} factors")
    return [robust_loss(x) for x in loss] if isinstance(loss, list) else [robust_loss(loss)] * n


def _upload_losses(losses, device):
    """(loss_kind int32 [n], loss_k float64 [n]) on the device from [(kind, k)]."""
    return (_upload(np.array([k for k, _ in losses], np.int32), device, torch.int32),
            _upload(np.array([k for _, k in losses], np.float64), device, torch.float64))


def _require_finite(what, sigmas, **values):
    """Refuse sigmas that are not finite and > 0, then any of the named `values` arrays that is not finite."""
    if not (np.isfinite(sigmas).all() and (sigmas > 0).all()):
        raise ValueError(f"{what}: sigmas must be finite and > 0")
    for name, v in values.items():
        if not np.isfinite(v).all():
            raise ValueError(f"{what}: {name} must be finite")


def _require_sqrt_info(what, R, n):
    """sqrt_info of n factors as [n, 6, 6]: finite, upper-triangular (every entry below the diagonal exactly 0) with a
    positive diagonal -- the R of include/vus_between.h with R^T R = cov^-1."""
    R = np.array(R, dtype=np.float64)
    if R.size != 36 * n or R.ndim not in (2, 3):
        raise ValueError(f"{what}: sqrt_info must be [n, 6, 6] or [n, 36] for n={n} factors, not an array of shape {R.shape}")
    R = R.reshape(n, 6, 6)
    if not np.isfinite(R).all():
        raise ValueError(f"{what}: sqrt_info must be finite")
    if np.tril(R, -1).any():
        f = int(np.nonzero(np.tril(R, -1).reshape(n, -1).any(axis=1))[0][0])
        raise ValueError(f"{what}: sqrt_info of factor {f} is not upper-triangular (an entry below the diagonal is not 0)")
    if not (np.diagonal(R, axis1=1, axis2=2) > 0).all():
        f = int(np.nonzero((np.diagonal(R, axis1=1, axis2=2) <= 0).any(axis=1))[0][0])
        raise ValueError(f"{what}: sqrt_info of factor {f} needs a positive diagonal")
    return R


def sqrt_info_of(covariances):
    """Per-factor covariances [n, 6, 6] (symmetric positive definite) -> (R [n, 6, 6], sigmas [n, 6]): R the upper Cholesky
    factor of cov^-1 (R^T R = cov^-1, positive diagonal), sigmas the roots of the covariance diagonals."""
    C = np.array(covariances, dtype=np.float64).reshape(-1, 6, 6)
    if not np.isfinite(C).all():
        raise ValueError("between factors: covariances must be finite")
    try:
        R = np.stack([np.linalg.cholesky(np.linalg.inv(c)).T for c in C]) if len(C) else np.zeros((0, 6, 6))
    except np.linalg.LinAlgError:
        raise ValueError("between factors: a covariance is not positive definite") from None
    return R, np.sqrt(np.diagonal(C, axis1=1, axis2=2))


def between_targets(node1, node2):
    """The CSR of include/vus_between.h on the host: every 6 x 6 block (node, s) of the band that BetweenFactorPose3 terms
    land in, ascending by (node, s), and per block its terms 4 f + kind in factor order (kind 0 J1^T J1 at (node1, 0),
    1 J2^T J2 at (node2, 0), 2 J1^T J2 at (node1, node1 - node2) when node1 > node2, 3 its transpose at (node2,
    node2 - node1) otherwise).  Returns (tgt_node, tgt_s, tgt_ptr, tgt_terms) as int32 arrays."""
    n1, n2 = np.asarray(node1, np.int64), np.asarray(node2, np.int64)
    f = np.arange(len(n1), dtype=np.int64)
    hi = n1 > n2
    node = np.concatenate([n1, n2, np.where(hi, n1, n2)])
    sdiag = np.concatenate([np.zeros_like(n1), np.zeros_like(n2), np.abs(n1 - n2)])
    term = np.concatenate([4 * f, 4 * f + 1, 4 * f + np.where(hi, 2, 3)])
    order = np.lexsort((term, sdiag, node))
    node, sdiag, term = node[order], sdiag[order], term[order]
    first = np.ones(len(node), bool)
    first[1:] = (node[1:] != node[:-1]) | (sdiag[1:] != sdiag[:-1])
    starts = np.nonzero(first)[0]
    ptr = np.append(starts, len(node))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(node[starts]), i32(sdiag[starts]), i32(ptr), i32(term)


class BetweenFactors:
    """Device-resident vus_between_factors: BetweenFactorPose3(X(i), X(j), meas, model) for i, j = `pose_i`, `pose_j`
    (either order, several on one pair allowed, i != j), meas [n, 12] flat12 of the measured T_i^-1 T_j, sigmas [n, 6]
    in the tangent order (omega, v).  `loss`: one robust model for all of them (robust_loss(): None = Gaussian) or a list
    (not a tuple) of n, one per factor (Gaussian odometry next to robust loop closures).  Node of pose p = pose_stride p.
    `span` = the widest pose distance, for StereoBAProblem(between_span=...).
    `max_span` (None: every factor is added to the band, which widens to the longest of them): factors that span MORE
    than max_span poses form the long set `.long` (a LongClosures, None if there is none) -- the solver keeps them out of
    the band and corrects every band solve by their low-rank term (include/vus_closure.h); this set then holds the rest
    (`n` may be 0) and `span` is the widest of the rest, so that between_span=span keeps the landmark band.
    `sqrt_info` (None: the diagonal models of `sigmas`, nothing else is uploaded): [n, 6, 6] or [n, 36], per factor the
    upper-triangular R with R^T R = cov^-1 of a full-covariance model (noiseModel.Gaussian); every factor then whitens with
    its R (a diagonal one carries diag(1/sigma)) and the rows of `sigmas` are not used.  BetweenFactors.from_covariances
    factors per-factor covariances on the host."""
    MAX_LONG = _abi.const("VUS_CLOSURE_MAX")

    @classmethod
    def from_covariances(cls, pose_i, pose_j, meas, covariances, n_poses, **kw):
        """The set under full-covariance models given as covariances [n, 6, 6] (tangent order (omega, v))."""
        R, sig = sqrt_info_of(covariances)
        return cls(pose_i, pose_j, meas, sig, n_poses, sqrt_info=R, **kw)

    def __init__(self, pose_i, pose_j, meas, sigmas, n_poses, pose_stride=1, loss=None, device="cuda:0", max_span=None,
                 sqrt_info=None):
        pi, pj = np.asarray(pose_i, np.int64).reshape(-1), np.asarray(pose_j, np.int64).reshape(-1)
        meas = np.asarray(meas, np.float64).reshape(-1, 12)
        sig = np.asarray(sigmas, np.float64).reshape(-1, 6)
        n = len(pi)
        if n == 0 or not (len(pj) == len(meas) == len(sig) == n):
            raise ValueError(f"between factors: {len(pi)} / {len(pj)} keys, {len(meas)} measurements, {len(sig)} sigmas")
        if ((pi < 0) | (pi >= n_poses) | (pj < 0) | (pj >= n_poses)).any():
            raise ValueError(f"between factors: a pose index outside [0, {n_poses})")
        if (pi == pj).any():
            f = int(np.nonzero(pi == pj)[0][0])
            raise ValueError(f"BetweenFactorPose3 {f} joins pose {int(pi[f])} to itself")
        _require_finite("between factors", sig)
        R = None if sqrt_info is None else _require_sqrt_info("between factors", sqrt_info, n)
        losses = _factor_losses(loss, n, "between factors")
        self.long = None
        if max_span is not None:
            far = np.abs(pi - pj) > int(max_span)
            if far.sum() > self.MAX_LONG:
                raise ValueError(f"between factors: {int(far.sum())} factors span more than max_span={int(max_span)} poses, "
                                 f"{self.MAX_LONG} long closures are supported: raise max_span (the band widens to it) or "
                                 "pass fewer closures")
            if far.any():
                self.long = LongClosures(pi[far], pj[far], meas[far], sig[far], n_poses, pose_stride,
                                         [l for l, f in zip(losses, far) if f], device,
                                         sqrt_info=None if R is None else R[far])
            pi, pj, meas, sig = pi[~far], pj[~far], meas[~far], sig[~far]
            R = None if R is None else R[~far]
            losses = [l for l, f in zip(losses, far) if not f]
            n = len(pi)
        self.n, self.n_poses, self.pose_stride = n, int(n_poses), int(pose_stride)
        self.span = int(np.abs(pi - pj).max()) if n else 0
        self.losses = losses
        self.host = dict(i=pi, j=pj, meas=meas, sigmas=sig, losses=self.losses, sqrt_info=R)
        if n == 0:          # every factor is a long closure: no in-band set, nothing to upload
            return
        dev = torch.device(device)
        t = lambda a, dt: _upload(a, dev, dt)
        ps = self.pose_stride
        self.node1, self.node2 = t(ps * pi, torch.int32), t(ps * pj, torch.int32)
        self.meas, self.w = t(meas, torch.float64), t(1.0 / sig, torch.float64)
        self.loss_kind, self.loss_k = _upload_losses(self.losses, dev)
        tn, ts, tp, tt = between_targets(ps * pi, ps * pj)
        self.tgt_node, self.tgt_s, self.tgt_ptr, self.tgt_terms = (t(a, torch.int32) for a in (tn, ts, tp, tt))
        p = _lib.ptr
        self.sqrt_info = None if R is None else t(R.reshape(n, 36), torch.float64)
        self.c = _CBetween(n, ps * self.n_poses, ps, p(self.node1), p(self.node2), p(self.meas), p(self.w),
                           p(self.loss_kind), p(self.loss_k), len(tn), p(self.tgt_node), p(self.tgt_s), p(self.tgt_ptr), p(self.tgt_terms),
                           None if R is None else p(self.sqrt_info))

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this set was not built for (the solver asks before it uses the set)."""
        if self.pose_stride != problem.pose_stride or self.n_poses != problem.n_poses:
            raise ValueError("BetweenFactors built for another problem (pose_stride / n_poses differ)")
        if self.span * problem.pose_stride > problem.band:
            raise ValueError(f"a between factor spans {self.span} poses, more than the problem's band of {problem.band} nodes: "
                             "build the StereoBAProblem with between_span=BetweenFactors.span")


class LongClosures(BetweenFactors):
    """The long set of a BetweenFactors(max_span=...): at most 64 between factors that stay out of the band.  The same
    vus_between_factors; the solver hands it to vus_closure_* and to vus_between_eval_step / vus_between_error."""

    def __init__(self, pose_i, pose_j, meas, sigmas, n_poses, pose_stride, losses, device, sqrt_info=None):
        super().__init__(pose_i, pose_j, meas, sigmas, n_poses, pose_stride, list(losses), device, sqrt_info=sqrt_info)
        self.min_span = int(np.abs(self.host["i"] - self.host["j"]).min())

    def _fits(self, problem):
        if self.pose_stride != problem.pose_stride or self.n_poses != problem.n_poses:
            raise ValueError("BetweenFactors built for another problem (pose_stride / n_poses differ)")
        if self.min_span * problem.pose_stride <= problem.band:
            raise ValueError(f"a long closure spans {self.min_span} poses, inside the problem's band of {problem.band} nodes: "
                             f"build the BetweenFactors with max_span >= {problem.band // problem.pose_stride}")


class PointPriors:
    """Device-resident vus_point_priors: PriorFactorPoint3(L(j), mean, model) for j = `point_idx` on landmarks of a
    StereoBAProblem with `n_points` landmarks; mean [n, 3], sigmas [n, 3] (a diagonal model; several priors on one landmark
    are summed).  The factors are sorted stably by landmark into the CSR on the host; `host` keeps them in that order.
    n = 0 is allowed and is the same as no PointPriors at all."""

    def __init__(self, point_idx, mean, sigmas, n_points, device="cuda:0"):
        idx = np.asarray(point_idx, np.int64).reshape(-1)
        mean = np.asarray(mean, np.float64).reshape(-1, 3)
        sig = np.asarray(sigmas, np.float64).reshape(-1, 3)
        n = len(idx)
        if not (len(mean) == len(sig) == n):
            raise ValueError(f"point priors: {n} landmark indices, {len(mean)} means, {len(sig)} sigmas")
        if ((idx < 0) | (idx >= n_points)).any():
            raise ValueError(f"point priors: a landmark index outside [0, {int(n_points)})")
        _require_finite("point priors", sig, means=mean)
        order, row_point, row_ptr = csr_rows(idx)
        self.n, self.n_points, self.n_rows = n, int(n_points), len(row_point)
        self.host = dict(idx=idx[order], mean=mean[order], sigmas=sig[order], row_point=row_point, row_ptr=row_ptr)
        dev = torch.device(device)
        t = lambda a, dt: _upload(a, dev, dt)
        self.row_point, self.row_ptr = t(row_point, torch.int32), t(row_ptr, torch.int32)
        self.mean, self.w = t(mean[order], torch.float64), t(1.0 / sig[order], torch.float64)
        p = (lambda x: _lib.ptr(x)) if n else (lambda x: None)
        self.c = _CPointPriors(n, self.n_points, self.n_rows, p(self.row_point), p(self.row_ptr), p(self.mean), p(self.w))

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this set was not built for (the solver asks before it uses the set)."""
        if self.n_points != problem.n_points:
            raise ValueError(f"PointPriors built for {self.n_points} landmarks, the problem has {problem.n_points}")


POSE_MEAS_POSITION, POSE_MEAS_ROTATION = _abi.const("VUS_POSE_MEAS_POSITION"), _abi.const("VUS_POSE_MEAS_ROTATION")


class PoseMeasurements:
    """Device-resident vus_pose_meas: partial absolute measurements on the poses X(i), i = `pose_idx`, of a problem with
    `n_poses` poses at `pose_stride`.  kind [n]: POSE_MEAS_POSITION (GPSFactor, GPSFactorArm, PoseTranslationPrior3D: `meas`
    row = the measured world position m (3), the lever arm a in the body frame (3), three zeros; r = t + R a - m) or
    POSE_MEAS_ROTATION (PoseRotationPrior3D: `meas` row = the measured rotation, row-major; r = Log(Rm^T R)).  sigmas [n, 3]
    (a diagonal model; a depth fix is a position fix with two wide sigmas).  `loss`: one robust model for all of them
    (robust_loss(): None = Gaussian) or a list (not a tuple) of n, one per factor.  Several factors on one pose, of
    either kind, are summed.  The factors are sorted stably by pose into the CSR on the host; `host` keeps them in that
    order and `order` maps a CSR slot to the factor's position in the input.  n = 0 is allowed and is the same as no
    PoseMeasurements at all."""

    def __init__(self, pose_idx, kind, meas, sigmas, n_poses, pose_stride=1, loss=None, device="cuda:0"):
        idx = np.asarray(pose_idx, np.int64).reshape(-1)
        kind = np.asarray(kind, np.int64).reshape(-1)
        meas = np.asarray(meas, np.float64).reshape(-1, 9)
        sig = np.asarray(sigmas, np.float64).reshape(-1, 3)
        n = len(idx)
        if not (len(kind) == len(meas) == len(sig) == n):
            raise ValueError(f"pose measurements: {n} pose indices, {len(kind)} kinds, {len(meas)} measurements, {len(sig)} sigmas")
        if ((idx < 0) | (idx >= n_poses)).any():
            raise ValueError(f"pose measurements: a pose index outside [0, {int(n_poses)})")
        if not np.isin(kind, (POSE_MEAS_POSITION, POSE_MEAS_ROTATION)).all():
            raise ValueError("pose measurements: kind must be POSE_MEAS_POSITION (0) or POSE_MEAS_ROTATION (1)")
        _require_finite("pose measurements", sig, measurements=meas)
        if int(pose_stride) not in (1, 2, 3):
            raise ValueError(f"pose_stride={pose_stride}: 1, 2 or 3")
        losses = _factor_losses(loss, n, "pose measurements")
        order, row_pose, row_ptr = csr_rows(idx)
        self.n, self.n_poses, self.pose_stride, self.n_rows = n, int(n_poses), int(pose_stride), len(row_pose)
        self.order = order
        self.losses = [losses[int(f)] for f in order]
        self.robust = any(k for k, _ in self.losses)
        self.host = dict(idx=idx[order], kind=kind[order], meas=meas[order], sigmas=sig[order], losses=self.losses,
                         row_pose=row_pose, row_ptr=row_ptr)
        dev = torch.device(device)
        t = lambda a, dt: _upload(a, dev, dt)
        self.row_pose, self.row_ptr = t(row_pose, torch.int32), t(row_ptr, torch.int32)
        self.kind = t(kind[order].astype(np.int32), torch.int32)
        self.meas, self.w = t(meas[order], torch.float64), t(1.0 / sig[order], torch.float64)
        self.loss_kind, self.loss_k = _upload_losses(self.losses, dev)
        p = (lambda x: _lib.ptr(x)) if n else (lambda x: None)
        self.c = _CPoseMeas(n, self.n_poses, self.pose_stride, self.n_rows, p(self.row_pose), p(self.row_ptr), p(self.kind),
                            p(self.meas), p(self.w), p(self.loss_kind), p(self.loss_k))

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this set was not built for (the solver asks before it uses the set)."""
        if self.pose_stride != problem.pose_stride or self.n_poses != problem.n_poses:
            raise ValueError(f"PoseMeasurements built for {self.n_poses} poses at pose_stride {self.pose_stride}, the "
                             f"problem has {problem.n_poses} at pose_stride {problem.pose_stride}")


class WindowPrior:
    """Device-resident vus_window_prior (include/vus_fixed_lag.h): a dense Gaussian prior over the m consecutive poses
    first .. first + m - 1 of a problem with `n_poses` poses at pose_stride 1 -- what a fixed-lag smoother leaves of the
    keyframes it has marginalised.  x0 [m, 12] the linearisation poses, H [6 m, 6 m] symmetric (positive semi-definite is
    enough), g [6 m] the gradient at x0, c the constant: error(x) = c + g^T d + 0.5 d^T H d with d the stack of
    Local(x0_i, x_i).  `span` = m - 1, for StereoBAProblem(between_span=...).  Arrays or device tensors are accepted; the
    library's check (the solver runs it) refuses a non-finite, asymmetric or negative-diagonal H."""

    def __init__(self, first, x0, H, g, c, n_poses, device="cuda:0"):
        dev = torch.device(device)
        self.x0 = _upload(x0, dev, torch.float64, (-1, 12))
        m = self.x0.shape[0]
        self.first, self.m, self.n_poses, self.c_const = int(first), int(m), int(n_poses), float(c)
        if m < 1:
            raise ValueError("window prior: at least one pose is needed")
        if self.first < 0 or self.first + m > self.n_poses:
            raise ValueError(f"window prior: poses {self.first} .. {self.first + m - 1} outside [0, {self.n_poses})")
        self.H = _upload(H, dev, torch.float64)
        self.g = _upload(g, dev, torch.float64).reshape(-1)
        if tuple(self.H.shape) != (6 * m, 6 * m) or self.g.numel() != 6 * m:
            raise ValueError(f"window prior: H {tuple(self.H.shape)} and g [{self.g.numel()}] for m={m} poses; "
                             f"[{6 * m}, {6 * m}] and [{6 * m}] are expected")
        self.n, self.span, self.pose_stride = 1, m - 1, 1
        p = _lib.ptr
        self.c = _CWindowPrior(self.n_poses, self.first, m, p(self.x0), p(self.H), p(self.g), self.c_const)

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this prior was not built for (the solver asks before it uses the prior)."""
        if problem.pose_stride != 1:
            raise ValueError(f"WindowPrior serves pose_stride 1 only, the problem has pose_stride {problem.pose_stride} "
                             "(inertial layouts are not supported)")
        if self.n_poses != problem.n_poses or self.first + self.m > problem.n_poses:
            raise ValueError(f"WindowPrior on poses {self.first} .. {self.first + self.m - 1} of {self.n_poses}, the problem "
                             f"has {problem.n_poses} poses")
        if self.m - 1 > problem.band:
            raise ValueError(f"the window prior spans {self.m - 1} poses, more than the problem's band of {problem.band} nodes: "
                             "build the StereoBAProblem with between_span=WindowPrior.span")


class NavWindowPrior:
    """Device-resident vus_nav_window_prior (include/vus_fixed_lag_nav.h): a dense Gaussian prior over pose, velocity and
    IMU bias of the m consecutive keyframes first .. first + m - 1 of a problem with `n_poses` keyframes in the
    per-keyframe-bias layout (pose_stride 3) -- what a fixed-lag smoother leaves of the inertial keyframes it has
    marginalised.  x0 [m, 12], v0 [m, 3], b0 [m, 6] the linearisation point, H [15 m, 15 m] symmetric (positive semi-definite
    is enough), g [15 m], c the constant: error = c + g^T d + 0.5 d^T H d with d per keyframe (Local(x0_i, x_i), v_i - v0_i,
    b_i - b0_i).  `span` = m - 1 KEYFRAMES; the band it needs is 3 m - 1 nodes (B of the last keyframe against X of the
    first), which StereoBAProblem(between_span=span + 1) at pose_stride 3 gives.  Arrays or device tensors are accepted; the library's check (the solver runs it) refuses a
    non-finite, asymmetric or negative-diagonal H."""

    def __init__(self, first, x0, v0, b0, H, g, c, n_poses, device="cuda:0"):
        dev = torch.device(device)
        self.x0 = _upload(x0, dev, torch.float64, (-1, 12))
        m = self.x0.shape[0]
        self.first, self.m, self.n_poses, self.c_const = int(first), int(m), int(n_poses), float(c)
        if m < 1:
            raise ValueError("nav window prior: at least one keyframe is needed")
        if self.first < 0 or self.first + m > self.n_poses:
            raise ValueError(f"nav window prior: keyframes {self.first} .. {self.first + m - 1} outside [0, {self.n_poses})")
        self.v0 = _upload(v0, dev, torch.float64, (-1, 3))
        self.b0 = _upload(b0, dev, torch.float64, (-1, 6))
        if self.v0.shape[0] != m or self.b0.shape[0] != m:
            raise ValueError(f"nav window prior: v0 {tuple(self.v0.shape)} and b0 {tuple(self.b0.shape)} for m={m} keyframes; "
                             f"[{m}, 3] and [{m}, 6] are expected")
        self.H = _upload(H, dev, torch.float64)
        self.g = _upload(g, dev, torch.float64).reshape(-1)
        if tuple(self.H.shape) != (15 * m, 15 * m) or self.g.numel() != 15 * m:
            raise ValueError(f"nav window prior: H {tuple(self.H.shape)} and g [{self.g.numel()}] for m={m} keyframes; "
                             f"[{15 * m}, {15 * m}] and [{15 * m}] are expected")
        self.n, self.span, self.pose_stride = 1, m - 1, 3
        p = _lib.ptr
        self.c = _CNavWindowPrior(self.n_poses, self.first, m, p(self.x0), p(self.v0), p(self.b0), p(self.H), p(self.g),
                                  self.c_const)

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this prior was not built for (the solver asks before it uses the prior)."""
        if problem.pose_stride != 3:
            raise ValueError(f"NavWindowPrior serves pose_stride 3 only (the per-keyframe-bias layout of NavBiasBASolver), the "
                             f"problem has pose_stride {problem.pose_stride}")
        if self.n_poses != problem.n_poses or self.first + self.m > problem.n_poses:
            raise ValueError(f"NavWindowPrior on keyframes {self.first} .. {self.first + self.m - 1} of {self.n_poses}, the "
                             f"problem has {problem.n_poses} poses")
        if 3 * self.m - 1 > problem.band:
            raise ValueError(f"the nav window prior spans {3 * self.m - 1} nodes, more than the problem's band of {problem.band} "
                             f"nodes: build the StereoBAProblem with between_span={self.m} (NavWindowPrior.span + 1 keyframes: "
                             "the band is 3 between_span nodes, and B of the last keyframe lies 3 m - 1 nodes from X of the first)")


@dataclass
class LMParams:
    """gtsam.LevenbergMarquardtParams() defaults."""
    lambdaInitial: float = 1e-5
    lambdaFactor: float = 10.0
    lambdaUpperBound: float = 1e5
    lambdaLowerBound: float = 0.0
    minModelFidelity: float = 1e-3
    maxIterations: int = 100
    relativeErrorTol: float = 1e-5
    absoluteErrorTol: float = 1e-5
    errorTol: float = 0.0
    diagonalDamping: bool = False
    useFixedLambdaFactor: bool = True


@dataclass
class LMReport:
    iterations: int = 0          # accepted steps (gtsam iterations())
    outer: int = 0               # linearisations
    tries: int = 0               # linear solves
    status: int = 1              # 0 converged, 1 max iterations, 2 lambda upper bound
    initial_error: float = 0.0
    final_error: float = 0.0
    final_lambda: float = 0.0
    err_hist: List[float] = field(default_factory=list)
    lambda_hist: List[float] = field(default_factory=list)
    seconds: float = 0.0
    setup_seconds: float = 0.0
    stereo_weights: Optional[tuple] = None     # gtsam shim, robust stereo factors: (pose keys, landmark keys, final w)
    pose_meas_weights: Optional[tuple] = None  # gtsam shim, a robust position / attitude fix: (pose keys, final w), graph order
    long_closures: int = 0       # between factors kept out of the band (BetweenFactors(max_span=...))
    closure_max_diag: float = 0.0  # largest max_i C_ii of a trial's capacitance matrix (vus_closure_diag_max); 0 without long closures
    closure_loss_trials: int = 0   # trials whose max_i C_ii exceeded StereoBASolver.CLOSURE_MAX_DIAG: their steps may have lost digits


def _i32(t):
    return t.to(torch.int32).contiguous()


def band_of(pk) -> int:
    """Widest keyframe span of a landmark = half-bandwidth, in pose blocks, of the reduced camera system."""
    band = pk.get("band")
    if band is None:
        if pk["n_obs"] == 0:
            return 0
        op, pptr = pk["obs_pose"], pk["point_ptr"].to(torch.int64)
        seen = pptr[1:] > pptr[:-1]
        first, last = op[pptr[:-1][seen]], op[pptr[1:][seen] - 1]
        band = int((last - first).max().item())
    return int(band)


def build_tiles_device(pk, band):
    """vus_ba_tiles of a packed problem (csrc/pack.hip: two launches and a radix sort): for every pair of 8-pose tiles
    within `band` poses of each other, the landmarks seen from both, in ascending order.  Returns a dict of device
    tensors + sizes; `band` >= the widest keyframe span of a landmark."""
    nP, nL, n_obs = pk["n_poses"], pk["n_points"], pk["n_obs"]
    dev = pk["obs_pose"].device
    n_tiles, dt1 = (nP + 7) // 8, (int(band) + 7) // 8 + 1
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"band": int(band), "n_tiles": n_tiles, "n_units": n_tiles * dt1, "n_entries": 0,
           "unit_ptr": torch.zeros(n_tiles * dt1 + 1, **i32), "order": torch.arange(n_tiles * dt1, **i32),
           "entries": torch.zeros((1, 4), **i32)}
    if n_obs == 0 or nL == 0:
        return out
    p, st_ptr = _lib.ptr, _lib.current_stream_ptr()
    cp = _CProblem(nP, nL, n_obs, 0, None, 1.0, None, p(pk["obs_pose"]), p(pk["obs_point"]), p(pk["point_ptr"]),
                   p(pk["obs_ppos"]), p(pk["pose_ptr"]), p(pk["pobs_lidx"]), None, None, None, 1)
    cnt = torch.empty(nL, **i32)
    base = torch.empty(nL + 1, **i32)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("vus_ba_tiles_count", ctypes.addressof(cp), p(cnt), st_ptr)
    _lib.call("vus_exclusive_scan_i32", p(cnt), nL, p(base), p(total), st_ptr)
    n = int(total.item())
    if n >= 2 ** 31:
        raise NotImplementedError(f"{n} tile-pair entries exceed the int32 entry index")
    out["n_entries"] = n
    out["entries"] = torch.empty((max(n, 1), 4), **i32)
    nbytes = int(_lib.load().vus_ba_tiles_work_bytes(n))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("vus_ba_tiles_fill", ctypes.addressof(cp), int(band), p(base), n, p(out["unit_ptr"]), p(out["entries"]),
              p(out["order"]), p(work), nbytes, st_ptr)
    return out


class StereoBAProblem:
    """Packed, device-resident stereo BA problem (vus_ba_problem + vus_ba_tiles).  `loss`: robust noise model of the
    stereo factors (robust_loss(): None = Gaussian, or e.g. ("cauchy", 2.0) with k in whitened units).  `between_span`: the
    widest pose distance of a BetweenFactorPose3 (BetweenFactors.span); the band in poses is the larger of it and the
    landmark span, scaled by pose_stride, so the tiles, Sband and the band-solve mode all follow the wider of the two.
    `body_P_sensor`: the camera-to-body extrinsic of every stereo factor (sensor_flat12(): a 12-vector, a 4 x 4 matrix or a
    gtsam.Pose3) -- the poses are then BODY poses and the left camera sits at pose o body_P_sensor; None = the poses are
    the camera's.
    `mono`: a bool / uint8 array per INPUT observation, nonzero = a monocular GenericProjectionFactor (include/vus_mono.h)
    whose `meas` row is (u, ignored, v) -- the middle slot is never used -- with the calibration `mono_K` = (fx, fy, skew,
    cx, cy) and the sigma `mono_sigma` of all of them.  K and sigma keep serving the stereo rows and are required even when
    every observation is mono.  None or all zero = a stereo-only problem, which calls the entry points it called before.
    `combined_imu` (pose_stride 3 only): the graph holds CombinedImuFactors, whose joint whitening couples B(i+1) with X(i),
    five nodes apart: the node band is then at least min(5, n_nodes - 1) instead of 4."""

    def __init__(self, obs_pose, obs_point, meas, n_poses, n_points, K, sigma, prior_pose=None,
                 prior_T=None, prior_sigmas=None, device="cuda:0", band=None, pose_stride=1, loss=None, between_span=0,
                 body_P_sensor=None, mono=None, mono_K=None, mono_sigma=None, combined_imu=False):
        _lib.require_gpu()
        _lib.load()
        dev = torch.device(device)
        t0 = time.perf_counter()

        def to_dev(x, dt):
            return torch.as_tensor(x).to(device=dev, dtype=dt).contiguous()
        if dev.type == "cuda":      # csrc/pack.hip: sorts and index arrays without torch's index operators
            pk = ba_pack.pack_observations_device(to_dev(obs_pose, torch.int32), to_dev(obs_point, torch.int32),
                                                  to_dev(meas, torch.float64), n_poses, n_points)
        else:
            pk = ba_pack.pack_observations(to_dev(obs_pose, torch.int64), to_dev(obs_point, torch.int64),
                                           to_dev(meas, torch.float64), n_poses, n_points)
        st = {"band": max(band_of(pk), int(between_span))}
        self.pk = pk
        self.device = dev
        self.n_poses, self.n_points, self.n_obs = int(n_poses), int(n_points), pk["n_obs"]
        self.pose_stride = int(pose_stride)
        self.n_nodes = self.pose_stride * int(n_poses)
        if self.pose_stride == 2:       # node layout with velocity nodes: pose blocks are 2 nodes apart,
            # inertial factors reach 3 nodes back, but no further than the graph's first node (a single keyframe: 1)
            st["band"] = min(max(self.pose_stride * st["band"], 3), self.n_nodes - 1)
        elif self.pose_stride == 3:     # velocity and bias nodes (NavBiasBASolver): an ImuFactor reaches 4 nodes back,
            # a CombinedImuFactor 5 (B(i+1) against X(i))
            st["band"] = min(max(self.pose_stride * st["band"], 5 if combined_imu else 4), self.n_nodes - 1)
        elif self.pose_stride > 3:
            raise ValueError(f"pose_stride={self.pose_stride}: 1, 2 or 3")
        if combined_imu and self.pose_stride != 3:
            raise ValueError(f"combined_imu=True needs pose_stride=3 (the per-keyframe-bias layout), not {self.pose_stride}")
        if band is not None:            # landmark-sharded solve: every rank allocates the global band
            if band < st["band"]:
                raise ValueError(f"band={band} is smaller than this problem's own band {st['band']}")
            st["band"] = int(band)
        self.band = st["band"]
        self.K = to_dev(K, torch.float64)
        assert self.K.numel() == 6
        self.sigma = float(sigma)
        self.loss = robust_loss(loss)
        self.robust = self.loss[0] != 0           # the Gaussian model keeps today's entry points
        self.c_loss = _CLoss(*self.loss)
        self.body_P_sensor = sensor_flat12(body_P_sensor)
        self.has_sensor = self.body_P_sensor is not None       # without one the entry points of today are called
        self.c_sensor = _CSensor((c_double * 12)(*self.body_P_sensor)) if self.has_sensor else None
        self._set_mono(mono, mono_K, mono_sigma)
        if prior_pose is None or len(prior_pose) == 0:
            self.prior_pose = torch.zeros(0, dtype=torch.int32, device=dev)
            self.prior_T = torch.zeros((0, 12), dtype=torch.float64, device=dev)
            self.prior_w = torch.zeros((0, 6), dtype=torch.float64, device=dev)
        else:
            self.prior_pose = to_dev(prior_pose, torch.int32)
            self.prior_T = to_dev(prior_T, torch.float64).reshape(-1, 12)
            # reciprocal on the host: a torch elementwise kernel used once here costs the first call of a process ~20 ms
            # of lazily loaded code objects (tools/cold_phases.py)
            ps = prior_sigmas.detach().cpu().numpy() if torch.is_tensor(prior_sigmas) else prior_sigmas
            self.prior_w = to_dev(1.0 / np.asarray(ps, dtype=np.float64).reshape(-1, 6), torch.float64)
        n_pr = self.prior_pose.numel()
        p = _lib.ptr
        self.c_problem = _CProblem(self.n_poses, self.n_points, self.n_obs, n_pr, p(self.K), 1.0 / self.sigma,
                                   p(pk["meas"]), p(pk["obs_pose"]), p(pk["obs_point"]), p(pk["point_ptr"]),
                                   p(pk["obs_ppos"]), p(pk["pose_ptr"]), p(pk["pobs_lidx"]),
                                   p(self.prior_pose) if n_pr else None, p(self.prior_T) if n_pr else None,
                                   p(self.prior_w) if n_pr else None, int(pose_stride))
        # the tile pairs the Schur kernel walks (their band is in POSES), built once per graph on the device
        self.tiles = tl = build_tiles_device(pk, self.band // self.pose_stride)
        self.c_tiles = _CTiles(tl["band"], tl["n_tiles"], tl["n_units"], tl["n_entries"], p(tl["unit_ptr"]),
                               p(tl["entries"]), p(tl["order"]))
        torch.cuda.synchronize(dev)
        self.setup_seconds = time.perf_counter() - t0


    def _set_mono(self, mono, mono_K, mono_sigma):
        """has_mono, is_mono_L (uint8 [n_obs], L-order: the input flags through the pack's `perm`) and the vus_ba_mono"""
        flags = None if mono is None else np.asarray(
            mono.detach().cpu().numpy() if torch.is_tensor(mono) else mono).reshape(-1) != 0
        self.has_mono = flags is not None and bool(flags.any())
        self.is_mono_L, self.c_mono, self.mono_K, self.mono_sigma = None, None, None, None
        if flags is not None and len(flags) != self.n_obs:
            raise ValueError(f"mono: {len(flags)} flags for {self.n_obs} observations")
        if not self.has_mono:
            return
        if mono_K is None or mono_sigma is None:
            raise ValueError("mono observations need mono_K = (fx, fy, skew, cx, cy) and mono_sigma")
        mk = np.array(mono_K.detach().cpu().numpy() if torch.is_tensor(mono_K) else mono_K, dtype=np.float64).reshape(-1)
        if mk.size != 5:
            raise ValueError(f"mono_K: (fx, fy, skew, cx, cy) is expected, not {mk.size} values")
        self.mono_K, self.mono_sigma = mk, float(mono_sigma)
        if not (np.isfinite(mk).all() and mk[0] > 0 and mk[1] > 0):
            raise ValueError(f"mono_K={mk.tolist()}: finite values with fx, fy > 0 are expected")
        if not (math.isfinite(self.mono_sigma) and self.mono_sigma > 0):
            raise ValueError(f"mono_sigma={self.mono_sigma} must be finite and > 0")
        perm = self.pk["perm"].cpu().numpy().astype(np.int64)
        self.is_mono_L = torch.from_numpy(flags[perm].astype(np.uint8)).to(self.device)
        self.c_mono = _CMono(_lib.ptr(self.is_mono_L), (c_double * 5)(*mk), 1.0 / self.mono_sigma)


class IndeterminantSystem(RuntimeError):
    """The information matrix at the linearisation point is not positive definite.  `kind` is "point" (landmark `index`
    has a singular 3 x 3 information block, e.g. every observation of it fails cheirality), "node" (the reduced camera
    system failed at camera-side node `index`) or "bias" (the shared-bias border is singular)."""

    def __init__(self, kind, index):
        super().__init__(f"indeterminant linear system at {kind} {index}")
        self.kind, self.index = kind, int(index)


class BAMarginals:
    """Marginal covariances at one linearisation point (StereoBASolver.marginals / NavBASolver.marginals), device tensors:
      Sigma     [n_nodes, band + 1, 36]  the band of the camera-side covariance (entry (i, s) = block (i, i - s)),
                                         border-corrected on inertial graphs
      pose_cov  [n_poses, 6, 6]          tangent order (rot, trans), body frame
      point_cov [n_points, 3, 3] or None world frame, indexed by the problem's landmark index
    and on inertial graphs vel_cov [n_poses, 3, 3], bias_cov [6, 6] (acc, gyro), node_bias_cov [n_nodes, 6, 6]; with one
    bias per keyframe (NavBiasBASolver) biases_cov [n_poses, 6, 6] instead of the last two (B(i) is node 3i + 2)."""

    def __init__(self, solver, values, Sigma, pose_cov, point_cov, U=None, vel_cov=None, bias_cov=None, node_bias_cov=None,
                 biases_cov=None):
        self.solver, self._values = solver, values
        self.biases_cov = biases_cov
        self.band, self.pose_stride = solver.P.band, solver.P.pose_stride
        self.Sigma, self.pose_cov, self.point_cov = Sigma, pose_cov, point_cov
        self.U, self.vel_cov, self.bias_cov, self.node_bias_cov = U, vel_cov, bias_cov, node_bias_cov

    def joint(self, nodes, bias=False):
        """Joint covariance [6m (+6), 6m (+6)] of the camera-side nodes `nodes` (pose i is node pose_stride * i), in the
        order given, with the shared bias appended last when `bias` (inertial graphs).  From the band when the nodes lie
        within `band` of each other, otherwise exactly from columns of S^-1 (a fresh lambda = 0 factorisation per 8
        columns, plus the border correction on inertial graphs)."""
        nodes = [int(q) for q in nodes]
        m = len(nodes)
        if bias and self.bias_cov is None:
            raise ValueError("bias=True needs an inertial graph (NavBASolver.marginals)")
        out = np.zeros((6 * m + 6 * bool(bias),) * 2)
        if m and max(nodes) - min(nodes) <= self.band:
            idx = torch.tensor([[max(a, b), max(a, b) - min(a, b)] for a in nodes for b in nodes], device=self.Sigma.device)
            blocks = self.Sigma[idx[:, 0], idx[:, 1]].reshape(m, m, 6, 6).cpu().numpy()
            for x, a in enumerate(nodes):
                for y, b in enumerate(nodes):
                    out[6 * x:6 * x + 6, 6 * y:6 * y + 6] = blocks[x, y] if a >= b else blocks[y, x].T
        elif m:
            out[:6 * m, :6 * m] = self.solver._exact_covariance_columns(self._values, nodes, self.U, self.node_bias_cov)
        if bias:
            nb = self.node_bias_cov[torch.tensor(nodes, dtype=torch.int64, device=self.Sigma.device)].cpu().numpy()
            out[:6 * m, 6 * m:] = nb.reshape(6 * m, 6) if m else 0.0
            out[6 * m:, :6 * m] = out[:6 * m, 6 * m:].T
            out[6 * m:, 6 * m:] = self.bias_cov.cpu().numpy()
        return out

    def joint_full(self, nodes, points=(), bias=False):
        """Joint covariance of camera-side nodes, landmarks (the problem's landmark indices) and, with `bias`, the shared
        bias, in the order nodes (6 each), bias (6), landmarks (3 each).  A landmark is l = -sum_k Y_kl^T x_k + e_l with
        e_l ~ N(0, V_l^-1) independent of the rest (Y = W V^-1 at lambda = 0), so the joint is M G M^T + diag(V_l^-1),
        G = the band's joint of every node involved.  Served when those nodes -- the requested ones and every pose
        observing a requested landmark -- lie within `band` of each other; otherwise NotImplementedError."""
        nodes, points = [int(q) for q in nodes], [int(j) for j in points]
        if not points:
            return self.joint(nodes, bias)
        rows = self.solver._point_rows(self._values, points)
        alln = sorted(set(nodes).union(*[set(r[1]) for r in rows]))
        if alln[-1] - alln[0] > self.band:
            raise NotImplementedError(
                f"joint covariance with landmarks: the camera-side nodes involved span {alln[-1] - alln[0]} nodes "
                f"({alln[0]} .. {alln[-1]}), more than the band of {self.band}; only joints inside one band window are served")
        G = self.joint(alln, bias)
        pos = {q: x for x, q in enumerate(alln)}
        m, nb = len(nodes), 6 * len(alln)
        r_lm = 6 * m + 6 * bool(bias)
        M = np.zeros((r_lm + 3 * len(points), G.shape[0]))
        for x, q in enumerate(nodes):
            M[6 * x:6 * x + 6, 6 * pos[q]:6 * pos[q] + 6] = np.eye(6)
        if bias:
            M[6 * m:6 * m + 6, nb:nb + 6] = np.eye(6)
        for t, (Y, onodes, _) in enumerate(rows):
            for y, q in zip(Y, onodes):
                M[r_lm + 3 * t:r_lm + 3 * t + 3, 6 * pos[q]:6 * pos[q] + 6] -= y.T
        C = M @ G @ M.T
        for t, (_, _, Vi) in enumerate(rows):
            C[r_lm + 3 * t:r_lm + 3 * t + 3, r_lm + 3 * t:r_lm + 3 * t + 3] += Vi
        return 0.5 * (C + C.T)


# One optional factor family of a solver: its stages over the LM state tuple (`assemble` takes lambda; a no-op where the
# family has no such stage) and `scal`, the view of its 4-double slot of the trial record.
_Term = namedtuple("_Term", "error linearize assemble eval_step scal")

# The buffers of one add-on family (between, point_prior, pose_meas) that is present: its factor object, `scal` again, the
# scalar of its stand-alone error and the workspace of vus_<family>_work_doubles.
_Family = namedtuple("_Family", "factors scal err work")


class StereoBASolver:
    """Workspace + LM loop.  Buffers are allocated once; optimize() allocates nothing."""

    def __init__(self, problem: StereoBAProblem, between: Optional[BetweenFactors] = None,
                 point_priors: Optional[PointPriors] = None, inertial=(), pose_meas: Optional[PoseMeasurements] = None,
                 window_prior: Optional[WindowPrior] = None):
        self.P = problem
        dev, nP, nL, nO, B = problem.device, problem.n_poses, problem.n_points, problem.n_obs, problem.band
        nN = problem.n_nodes                       # camera-side nodes (= poses unless velocity nodes are interleaved)
        f64 = dict(dtype=torch.float64, device=dev)
        self.W = torch.empty((nO, 18), **f64)
        self.V = torch.empty((nL, 6), **f64)
        self.Vinv = torch.empty((nL, 6), **f64)
        self.gl = torch.empty((nL, 3), **f64)
        self.dl = torch.empty((nL, 3), **f64)
        self.Hpp = torch.empty((nP, 36), **f64)
        self.gp = torch.empty((nP, 6), **f64)
        self.gs = torch.empty((nN, 6), **f64)
        self.dp = torch.empty((nN, 6), **f64)
        self.Sband = torch.empty((nN, B + 1, 36), **f64)
        self.new_poses = torch.empty((nP, 12), **f64)
        self.new_points = torch.empty((nL, 3), **f64)
        self.work = torch.empty((2 * (nL + 1) + 8,), **f64)
        self.Q = point_priors if point_priors is not None and point_priors.n else None      # no factors: no hooks
        self.M = pose_meas if pose_meas is not None and pose_meas.n else None
        self.B = between if between is not None and between.n else None       # the in-band set
        self.C = between.long if between is not None else None                # the long set (LongClosures) or None
        # the dense prior over a window or None: over poses (pose_stride 1) or over poses, velocities and biases (3)
        self.WP = window_prior if not isinstance(window_prior, NavWindowPrior) else None
        self.NWP = window_prior if isinstance(window_prior, NavWindowPrior) else None
        self._closure_loss_trials, self._closure_max_diag = 0, 0.0            # what _lm_eval has seen (CLOSURE_MAX_DIAG)
        # The add-on factor families, each described once: (C name: its entry points are vus_<name>_<stage>, its hooks
        # <name>_<stage>; the factor object or None; the name of its slot view; the state tensor its stages read, 0 poses
        # or -1 points, or a slice of several (each one argument of the hook); the arguments of its vus_<name>_check after the factors; whether it has an assemble stage).  The
        # terms are the families present in this, the canonical order -- between, long closures, the window prior (of either
        # layout), landmark priors, pose measurements --
        # and then the inertial ones (`inertial`: the stages an inertial subclass passes, as (name of the slot view, error,
        # linearize, assemble, eval_step)).  Every stage runs the stereo step first and then the terms in this order,
        # which is what keeps:
        #   - linearize() before the landmark priors' linearize, which adds into V and gl; both before schur() and
        #     before _check_points (a prior can make a landmark determinate)
        #   - linearize(), which WRITES Hpp and gp, before the pose measurements' linearize, which adds into them, and that
        #     before schur(), which reads them.  The pose measurements have no assemble stage and touch nothing the other
        #     terms read, so their place among the terms is free: they stand next to the landmark priors, the other family
        #     that enters before the Schur step, and the inertial terms a subclass passes stay last
        #   - between_assemble() and closure_assemble() (the long set's gradient) after schur() and before the inertial
        #     assemble, which copies gs into its right-hand side
        #   - eval_step() before every other eval_step: they read new_poses / new_points
        families = [f for f in (("between", self.B, "btw_scal", 0, (B,), True),
                                ("closure", self.C, "clo_scal", 0, (B,), True),
                                ("window_prior", self.WP, "wp_scal", 0, (B,), True),
                                ("nav_window_prior", self.NWP, "nwp_scal", slice(0, 3), (B,), True),
                                ("point_prior", self.Q, "pp_scal", -1, (), False),
                                ("pose_meas", self.M, "pm_scal", 0, (), False)) if f[1] is not None]

        def term(name, slot, at, assembles):
            pick = (lambda s: s[at]) if isinstance(at, slice) else (lambda s: (s[at],))
            stage = lambda st: lambda s: getattr(self, f"{name}_{st}")(*pick(s))       # the public hook, on its state tensor(s)
            assemble = (lambda lam: getattr(self, f"{name}_assemble")()) if assembles else (lambda lam: None)
            # the nav window prior reads new_vels and new_bias, which the inertial eval_step writes: that term runs it
            evaluate = (lambda s: None) if name == "nav_window_prior" else stage("eval_step")
            return slot, stage("error"), stage("linearize"), assemble, evaluate

        terms = [term(name, slot, at, assembles) for name, _, slot, at, _, assembles in families] + list(inertial)
        # one record per lambda trial, read back with ONE device-to-host copy: [0] linearise error, [1] linearised error
        # at the step, [2] new error, [3] spare, [4] (as two int32) the band solve's status word, then one slot of 4 per
        # term in list order: its three errors in the same order and a spare
        self._trial = torch.zeros((5 + 4 * len(terms),), **f64)
        self.scal = self._trial[:4]
        self.status = self._trial[4:5].view(torch.int32)[:1]
        self._terms = []
        for i, (name, *stages) in enumerate(terms):
            slot = self._trial[5 + 4 * i:9 + 4 * i]
            setattr(self, name, slot)
            if name == "clo_scal":
                self._clo_at = 5 + 4 * i
            self._terms.append(_Term(*stages, slot))
        self._families = {}
        for name, factors, slot, _, check_args, _ in families:
            factors._fits(problem)
            work = torch.empty((int(getattr(_lib.load(), f"vus_{name}_work_doubles")(factors.addr())),), **f64)
            self._families[name] = _Family(factors, getattr(self, slot), torch.empty((1,), **f64), work)
            if factors is self.B:
                self.btw_lin = torch.empty((factors.n, 120), **f64)
            if factors is self.WP:      # the gradient g + H delta at the linearisation
                self.wp_grad = torch.empty((6 * factors.m,), **f64)
            if factors is self.NWP:
                self.nwp_grad = torch.empty((15 * factors.m,), **f64)
            if factors is self.C:       # rows of [J1 J2 r]; U, overwritten by Z = B^-1 U; C = I + U^T Z and its factor
                self.clo_rows = torch.empty((factors.n, 78), **f64)
                self.clo_UZ = torch.empty((6 * factors.n, 6 * nN), **f64)
                self.clo_C = torch.empty((6 * factors.n, 6 * factors.n), **f64)
            _lib.call(f"vus_{name}_check", factors.addr(), *check_args, _lib.current_stream_ptr())
        # two-sided band solve (vus_ba_band_solve_split): worth it once the chain of panel steps is much longer than
        # the band; its workspace (pose-reversed copy of the lower half + the middle system) is allocated once
        self.band_rhs = 1
        self._alloc_band_work()
        self._unit_counter = torch.zeros(1, dtype=torch.int32, device=dev)      # the Schur kernel's unit queue

    SPLIT_MIN_EXTRA = 64       # use the two-sided solve when n_nodes >= 2 * band + this

    def _alloc_band_work(self):
        nN, B = self.P.n_nodes, self.P.band
        n = int(_lib.load().vus_ba_band_solve_work_doubles(nN, B, self.band_rhs))
        # the long closures' correction reads the factor the solve leaves in Sband: the split solves leave it unspecified
        self.use_split = n > 0 and nN >= 2 * B + self.SPLIT_MIN_EXTRA and self.C is None
        self.band_work = torch.empty((n if self.use_split else 0,), dtype=torch.float64, device=self.P.device)

    # -- single kernels (also used by the parity tests) ------------------------------------------
    def _pp(self):
        return ctypes.addressof(self.P.c_problem)

    def _loss_args(self, name):
        """(entry point, trailing arguments): the `_robust` twin with the problem's vus_ba_loss for a robust model; with a
        body_P_sensor the `_sensor` form, which takes the loss (Gaussian included) and the extrinsic; with monocular
        observations the `_mixed` form, which takes the loss, the extrinsic or NULL, and the vus_ba_mono"""
        if self.P.has_mono:
            return name + "_mixed", (ctypes.addressof(self.P.c_loss),
                                     ctypes.addressof(self.P.c_sensor) if self.P.has_sensor else None,
                                     ctypes.addressof(self.P.c_mono))
        if self.P.has_sensor:
            return name + "_sensor", (ctypes.addressof(self.P.c_loss), ctypes.addressof(self.P.c_sensor))
        return (name + "_robust", (ctypes.addressof(self.P.c_loss),)) if self.P.robust else (name, ())

    def error(self, poses, points) -> float:
        """Nonlinear error of the stereo factors (sum of rho(d) under a robust model) and priors."""
        fn, extra = self._loss_args("vus_ba_error")
        _lib.call(fn, self._pp(), _lib.ptr(poses), _lib.ptr(points), _lib.ptr(self.scal),
                  _lib.ptr(self.work), _lib.current_stream_ptr(), *extra)
        return float(self.scal[0].item())

    def linearize(self, poses, points):
        """scal[0] = the linear system's error at delta = 0 (0.5 sum w d^2 under a robust model)."""
        p = _lib.ptr
        fn, extra = self._loss_args("vus_ba_linearize")
        _lib.call(fn, self._pp(), p(poses), p(points), p(self.W), p(self.V), p(self.gl),
                  p(self.Hpp), p(self.gp), p(self.scal), p(self.work), _lib.current_stream_ptr(), *extra)

    def stereo_weights(self, poses, points) -> torch.Tensor:
        """Robust weight w(d) of every observation, stereo or mono, at (poses, points), in the problem's INPUT row order
        (all ones under the Gaussian model): inliers near 1, gross outliers near 0."""
        w = torch.empty(self.P.n_obs, dtype=torch.float64, device=self.P.device)
        plain = not (self.P.has_sensor or self.P.has_mono)
        fn, extra = ("vus_ba_stereo_weights", ()) if plain else self._loss_args("vus_ba_stereo_weights")
        _lib.call(fn, self._pp(), ctypes.addressof(self.P.c_loss), _lib.ptr(poses), _lib.ptr(points),
                  _lib.ptr(w), _lib.current_stream_ptr(), *extra[1:])
        out = torch.empty_like(w)
        out[self.P.pk["perm"].to(torch.int64)] = w               # perm: L-order row -> input row
        return out

    def schur(self, lam: float, Y=None):
        """Y: optional [n_obs,18] buffer that receives W Vinv (L-order); the kernel forms it on the fly and needs no
        such array (288 MB at configs[2])."""
        p = _lib.ptr
        _lib.call("vus_ba_schur", self._pp(), ctypes.addressof(self.P.c_tiles), float(lam), p(self.W), p(self.V),
                  p(self.gl), p(self.Hpp), p(self.gp), p(self.Vinv), p(Y), p(self.Sband), self.P.band, p(self.gs),
                  p(self._unit_counter), _lib.current_stream_ptr())

    def band_solve(self):
        p = _lib.ptr
        if self.use_split:
            _lib.call("vus_ba_band_solve_split", p(self.Sband), self.P.n_nodes, self.P.band, p(self.gs), p(self.dp),
                      p(self.status), p(self.band_work), _lib.current_stream_ptr())
        else:
            _lib.call("vus_ba_band_solve", p(self.Sband), self.P.n_nodes, self.P.band, p(self.gs), p(self.dp),
                      p(self.status), _lib.current_stream_ptr())

    def _window_expired(self, status) -> bool:
        """True if the trial should be redone: the persistent window kernel (band mode 3) gave up a bounded wait
        (VUS_STATUS_WINDOW_EXPIRED) -- its flag protocol needs every workgroup of its launch resident at once, and other
        work on the device (another rank or process on this GPU, a kernel of another stream holding CUs) can prevent
        that.  The launch-pair mode has no such demand: it is latched for the rest of the process (vus_ba_set_tuning is
        process-wide) and the caller redoes Schur + solve.  Every rank of a sharded solve sees the same status word and
        takes the same branch.  An expired wait under a mode the caller FORCED, or a second failure, is raised."""
        lib = _lib.load()
        if status != _lib.STATUS_WINDOW_EXPIRED or lib.vus_ba_get_tuning(_lib.TUNE_BAND_MODE) >= 0:
            return False
        import warnings
        warnings.warn("vus band solve: the persistent window kernel could not keep its workgroups resident (is other work "
                      "running on this GPU?); falling back to the launch-pair factorisation for the rest of the process")
        _lib.call("vus_ba_set_tuning", _lib.TUNE_BAND_MODE, 2)
        self.window_fallbacks = getattr(self, "window_fallbacks", 0) + 1
        return True

    def backsub(self):
        p = _lib.ptr
        _lib.call("vus_ba_backsub", self._pp(), p(self.W), p(self.Vinv), p(self.gl), p(self.dp), p(self.dl),
                  _lib.current_stream_ptr())

    def eval_step(self, poses, points):
        p = _lib.ptr
        fn, extra = self._loss_args("vus_ba_eval_step")
        _lib.call(fn, self._pp(), p(poses), p(points), p(self.dp), p(self.dl), p(self.new_poses),
                  p(self.new_points), p(self.scal[1:]), p(self.work), _lib.current_stream_ptr(), *extra)

    # -- the add-on families: between factors (include/vus_between.h), priors on observed landmarks
    # (include/vus_point_prior.h), position / attitude fixes on poses (include/vus_pose_meas.h).  Every hook is a no-op
    # without its family.
    def _family_call(self, name, stage, args) -> bool:
        """vus_<name>_<stage>(factors, *args(family), stream) if the family is present -- `args` maps its _Family to the
        arguments in between, tensors standing for their device pointers -- and whether it is."""
        fam = self._families.get(name)
        if fam is not None:
            _lib.call(f"vus_{name}_{stage}", fam.factors.addr(), *(_lib.ptr(a) if torch.is_tensor(a) else a for a in args(fam)),
                      _lib.current_stream_ptr())
        return fam is not None

    def _family_error(self, name, x) -> float:
        ran = self._family_call(name, "error", lambda f: (x, f.err, f.work))
        return float(self._families[name].err[0].item()) if ran else 0.0

    def between_error(self, poses) -> float:
        """Error (sum rho under a robust model) of the between factors at poses; 0.0 without them."""
        return self._family_error("between", poses)

    def between_linearize(self, poses):
        """btw_lin = the per-factor products, btw_scal[0] = their linear error at delta = 0."""
        self._family_call("between", "linearize", lambda f: (poses, self.btw_lin, f.scal, f.work))

    def between_assemble(self):
        """Sband += the between blocks, gs += their gradient: after schur(), before an inertial assemble."""
        self._family_call("between", "assemble", lambda f: (self.btw_lin, self.P.band, self.Sband, self.gs))

    def between_eval_step(self, poses):
        """btw_scal[1] = linearised error at the step dp, btw_scal[2] = error at new_poses (after eval_step)."""
        self._family_call("between", "eval_step", lambda f: (poses, self.dp, self.new_poses, f.scal[1:], f.work))

    # The long set (include/vus_closure.h): its error and step evaluation are the between factors' own entry points on
    # the long set; linearize keeps the whitened Jacobian rows, assemble adds only their gradient, and the blocks enter
    # through _closure_correct after the band solve.
    def _closure_call(self, fn, args) -> bool:
        fam = self._families.get("closure")
        if fam is not None:
            _lib.call(fn, fam.factors.addr(), *(_lib.ptr(a) if torch.is_tensor(a) else a for a in args(fam)),
                      _lib.current_stream_ptr())
        return fam is not None

    def closure_error(self, poses) -> float:
        """Error (sum rho under a robust model) of the long closures at poses; 0.0 without them."""
        ran = self._closure_call("vus_between_error", lambda f: (poses, f.err, f.work))
        return float(self._families["closure"].err[0].item()) if ran else 0.0

    def closure_linearize(self, poses):
        """clo_rows = [J1 J2 r] of every long closure, clo_scal[0] = their linear error at delta = 0."""
        self._closure_call("vus_closure_linearize", lambda f: (poses, self.clo_rows, f.scal, f.work))

    def closure_assemble(self):
        """gs += the long closures' gradient (Sband receives nothing of them): where between_assemble() stands."""
        self._closure_call("vus_closure_gradient", lambda f: (self.clo_rows, self.gs))

    def closure_eval_step(self, poses):
        """clo_scal[1] = linearised error at the step dp, clo_scal[2] = error at new_poses (after eval_step)."""
        self._closure_call("vus_between_eval_step", lambda f: (poses, self.dp, self.new_poses, f.scal[1:], f.work))

    # max_i C_ii above which LMReport.closure_loss_trials counts a trial.  The correction cancels the band solution by about
    # that factor: where an odometry dropout leaves the band system held by lambda alone and a long closure bridges it, C_ii
    # grows like 1 / lambda and the step loses as many digits against the widened band.  profiles/closure_conditioning.md: on
    # the CPU sweep of tests/closure_cond_ref.py the low-rank solve keeps the widened band's accuracy up to max C_ii = 1.12e8;
    # a quarter of it.  The trial is counted, not refused: a heavy closure on a sound band system has a large C_ii as well
    # and loses nothing against the widened band (the profile has both cases).
    CLOSURE_MAX_DIAG = 2.8e7

    def _closure_correct(self, X, n_rhs):
        """X [n_rhs, 6 n_nodes], solved against the band system whose one-sided factor is in Sband, becomes the solution
        with the long closures: Z = B^-1 U (vus_ba_band_resolve), C = I + U^T Z, X -= Z C^-1 U^T X.  No-op without them.
        clo_scal[3] = max_i C_ii (vus_closure_diag_max), which _lm_eval records and holds against CLOSURE_MAX_DIAG."""
        if self.C is None:
            return
        nN, B = self.P.n_nodes, self.P.band
        self._closure_call("vus_closure_scatter", lambda f: (self.clo_rows, self.clo_UZ))
        _lib.call("vus_ba_band_resolve", _lib.ptr(self.Sband), nN, B, _lib.ptr(self.clo_UZ), 6 * self.C.n, None, 0,
                  _lib.current_stream_ptr())
        self._closure_call("vus_closure_capacitance", lambda f: (self.clo_rows, self.clo_UZ, self.clo_C))
        self._closure_call("vus_closure_diag_max", lambda f: (self.clo_C, f.scal[3:]))      # the slot's spare: _lm_eval reads it
        self._closure_call("vus_closure_correct", lambda f: (self.clo_rows, self.clo_UZ, self.clo_C, X, n_rhs, f.work))

    def _refuse_long(self, what):
        if self.C is not None:
            raise NotImplementedError(f"{what} with long closures (BetweenFactors(max_span=...)) is not implemented: the band "
                                      "of the covariance needs a rank-6k update; build the factors without max_span")

    # The dense prior over a pose window (include/vus_fixed_lag.h): what a fixed-lag smoother leaves of marginalised keyframes.
    def window_prior_error(self, poses) -> float:
        """Error c + g^T d + 0.5 d^T H d of the window prior at poses; 0.0 without one."""
        return self._family_error("window_prior", poses)

    def window_prior_linearize(self, poses):
        """wp_grad = g + H delta, wp_scal[0] = the prior's error at poses (its linear error at a zero step)."""
        self._family_call("window_prior", "linearize", lambda f: (poses, self.wp_grad, f.scal, f.work))

    def window_prior_assemble(self):
        """Sband += the blocks of H, gs += wp_grad: after schur(), before an inertial assemble."""
        self._family_call("window_prior", "assemble", lambda f: (self.wp_grad, self.P.band, self.Sband, self.gs))

    def window_prior_eval_step(self, poses):
        """wp_scal[1] = linearised error at the step dp, wp_scal[2] = error at new_poses (after eval_step)."""
        self._family_call("window_prior", "eval_step", lambda f: (poses, self.dp, self.new_poses, f.scal[1:], f.work))

    # The same over an inertial window (include/vus_fixed_lag_nav.h): poses, velocities and per-keyframe biases.
    def nav_window_prior_error(self, poses, vels, biases) -> float:
        """Error of the nav window prior at (poses, vels, biases); 0.0 without one."""
        ran = self._family_call("nav_window_prior", "error", lambda f: (poses, vels, biases, f.err, f.work))
        return float(self._families["nav_window_prior"].err[0].item()) if ran else 0.0

    def nav_window_prior_linearize(self, poses, vels, biases):
        """nwp_grad = g + H delta, nwp_scal[0] = the prior's error at the state (its linear error at a zero step)."""
        self._family_call("nav_window_prior", "linearize", lambda f: (poses, vels, biases, self.nwp_grad, f.scal, f.work))

    def nav_window_prior_assemble(self):
        """Sband += the entries of H, gs += nwp_grad: after schur(), before the inertial assemble."""
        self._family_call("nav_window_prior", "assemble", lambda f: (self.nwp_grad, self.P.band, self.Sband, self.gs))

    def nav_window_prior_eval_step(self, poses, vels, biases):
        """nwp_scal[1] = linearised error at the step dp, nwp_scal[2] = error at the new state: after eval_step AND the
        inertial eval_step, which writes new_vels and new_bias (the inertial term runs it, not the term list)."""
        self._family_call("nav_window_prior", "eval_step", lambda f: (poses, vels, biases, self.dp, self.new_poses, self.new_vels,
                                                                     self.new_bias, f.scal[1:], f.work))

    def marginalize_head(self, poses, points, n_drop) -> WindowPrior:
        """Eliminate every landmark and the first `n_drop` poses of THIS solver's problem at (poses, points) and return the
        Gaussian prior that leaves on its remaining poses n_drop .. n_poses - 1: a WindowPrior with first = 0,
        m = n_poses - n_drop and x0 = poses[n_drop:], for a problem of those m poses.  The solver is one built from exactly
        the factors to be absorbed (choosing them is the smoother's job); nothing of it is changed.  The linear system is
        the one marginals() uses -- no damping, the robust weights of that point; H = S_RR - S_RM S_MM^-1 S_MR and
        g = g_R - S_RM S_MM^-1 g_M from vus_ba_band_marginalize, and c = the linear error at a zero step of all terms
        - 0.5 g_M^T S_MM^-1 g_M - 0.5 sum_l gl_l^T V_l^-1 gl_l, the minimum of the linearised cost over everything eliminated.
        Raises IndeterminantSystem("point", j) / ("node", i) where the eliminated part is not positive definite."""
        self._refuse_long("marginalize_head()")
        if self.P.pose_stride != 1:
            raise NotImplementedError("marginalize_head() serves pose_stride 1 only (inertial layouts are not supported)")
        nN, B, k = self.P.n_nodes, self.P.band, int(n_drop)
        if not 1 <= k < nN:
            raise ValueError(f"marginalize_head: n_drop={k} outside [1, n_poses={nN})")
        if nN - k > B + 1:
            raise ValueError(f"marginalize_head: the {nN - k} remaining poses do not fit the band of {B} nodes: build the "
                             f"StereoBAProblem with between_span={nN - k - 1}")
        values = (poses.to(torch.float64).contiguous(), points.to(torch.float64).contiguous())
        self._linearize_all(values)
        self._assemble_zero()
        n = 6 * (nN - k)
        f64 = dict(dtype=torch.float64, device=self.P.device)
        H, g, quad = torch.empty((n, n), **f64), torch.empty((n,), **f64), torch.empty((1,), **f64)
        status = torch.empty((1,), dtype=torch.int32, device=self.P.device)
        work = torch.empty((int(_lib.load().vus_ba_band_marginalize_work_doubles(nN, B, k)),), **f64)
        p = _lib.ptr
        _lib.call("vus_ba_band_marginalize", p(self.Sband), nN, B, p(self.gs), k, p(H), p(g), p(quad), p(status), p(work),
                  _lib.current_stream_ptr())
        bad = int(status.item())
        if bad > 0:
            raise IndeterminantSystem("node", (bad - 1) // 6)
        lin0 = self._trial_errors(self._trial.cpu())[0]
        land = 0.0
        if self.P.n_points:     # gl^T V^-1 gl per landmark; Vinv is what the Schur step at lambda = 0 left (upper triangle)
            vi, gl = self.Vinv, self.gl
            x, y, z = gl[:, 0], gl[:, 1], gl[:, 2]
            land = float((vi[:, 0] * x * x + vi[:, 3] * y * y + vi[:, 5] * z * z
                          + 2.0 * (vi[:, 1] * x * y + vi[:, 2] * x * z + vi[:, 4] * y * z)).sum().item())
        c = lin0 - 0.5 * float(quad.item()) - 0.5 * land
        return WindowPrior(0, values[0][k:], H, g, c, nN - k, device=self.P.device)

    def point_prior_error(self, points) -> float:
        """Error of the landmark priors at points; 0.0 without them."""
        return self._family_error("point_prior", points)

    def point_prior_linearize(self, points):
        """V, gl += the landmark priors at points, pp_scal[0] = their error: after linearize(), before schur()."""
        self._family_call("point_prior", "linearize", lambda f: (points, self.V, self.gl, f.scal, f.work))

    def point_prior_eval_step(self, points):
        """pp_scal[1] = the priors' error at points + dl, pp_scal[2] = at new_points (after eval_step)."""
        self._family_call("point_prior", "eval_step", lambda f: (points, self.dl, self.new_points, f.scal[1:], f.work))

    def pose_meas_error(self, poses) -> float:
        """Error (sum rho under a robust model) of the pose measurements at poses; 0.0 without them."""
        return self._family_error("pose_meas", poses)

    def pose_meas_linearize(self, poses):
        """Hpp, gp += the pose measurements at poses, pm_scal[0] = their linear error at delta = 0: after linearize(),
        before schur()."""
        self._family_call("pose_meas", "linearize", lambda f: (poses, self.Hpp, self.gp, f.scal, f.work))

    def pose_meas_eval_step(self, poses):
        """pm_scal[1] = linearised error at the step dp, pm_scal[2] = error at new_poses (after eval_step)."""
        self._family_call("pose_meas", "eval_step", lambda f: (poses, self.dp, self.new_poses, f.scal[1:], f.work))

    def pose_meas_weights(self, poses) -> Optional[torch.Tensor]:
        """Robust weight w(d) of every pose measurement at poses, in the order the PoseMeasurements were GIVEN (all ones
        for Gaussian factors); None without them."""
        if self.M is None:
            return None
        w = torch.empty(self.M.n, dtype=torch.float64, device=self.P.device)
        self._family_call("pose_meas", "weights", lambda f: (poses, w))
        out = torch.empty_like(w)
        out[torch.from_numpy(self.M.order).to(self.P.device)] = w            # order: CSR slot -> input position
        return out

    def _trial_errors(self, rec):
        """[linearise error, linearised error at the step, new error] from one trial record: the stereo factors' and pose
        priors', plus every term's in list order"""
        v = rec.tolist()
        return [sum((v[slot + k] for slot in range(5, len(v), 4)), v[k]) for k in range(3)]

    # -- marginal covariances (gtsam.Marginals) ---------------------------------------------------------------------
    def _check_points(self):
        """Refuse a landmark whose information block is not positive definite before it is inverted at lambda = 0."""
        if self.P.n_points == 0:
            return
        bad = torch.empty(1, dtype=torch.int32, device=self.P.device)
        _lib.call("vus_ba_point_check", _lib.ptr(self.V), self.P.n_points, _lib.ptr(bad), _lib.current_stream_ptr())
        j = int(bad.item())
        if j != 0x7F7F7F7F:
            raise IndeterminantSystem("point", j)

    def _factor_status(self):
        """Status of the last factorisation: True to redo it (window kernel fallback), raises on a non-PD system."""
        status = int(self.status.item())
        if status < 0:
            if self._window_expired(status):
                return True
            raise RuntimeError("vus_ba_band_solve: the cooperative back-substitution timed out (status %d)" % status)
        if status > 0:
            raise IndeterminantSystem("node", (status - 1) // 6)
        return False

    def _marginal_factor(self, values):
        """Linearise at `values` with no damping and leave the ONE-SIDED factor of S (lambda = 0) in Sband, redoing the
        factorisation after a window-kernel fallback."""
        self._linearize_all(values)
        while True:
            self._assemble_zero()
            self._factor_zero()
            if not self._factor_status():
                return

    def _factor_zero(self):
        p = _lib.ptr
        _lib.call("vus_ba_band_solve", p(self.Sband), self.P.n_nodes, self.P.band, p(self.gs), p(self.dp),
                  p(self.status), _lib.current_stream_ptr())

    def _selinv(self):
        nN, B = self.P.n_nodes, self.P.band
        nw = int(_lib.load().vus_ba_band_selinv_work_doubles(nN, B))
        if getattr(self, "_selinv_work", None) is None:       # allocated on the first marginals() call, then reused
            self._selinv_work = torch.empty((nw,), dtype=torch.float64, device=self.P.device)
        Sigma = torch.empty_like(self.Sband)
        _lib.call("vus_ba_band_selinv", _lib.ptr(self.Sband), nN, B, _lib.ptr(Sigma), _lib.ptr(self._selinv_work), nw,
                  _lib.current_stream_ptr())
        return Sigma

    def _point_rows(self, values, points):
        """Per landmark j of `points`: (Y rows [m, 6, 3] = W V^-1 at lambda = 0, the camera-side nodes of its observations,
        V_j^-1) at `values`, from a fresh stereo linearisation (robust weights and landmark priors included)."""
        self.linearize(values[0], values[-1])
        self.point_prior_linearize(values[-1])
        ptr = self.P.pk["point_ptr"].cpu().numpy()
        obs_pose = self.P.pk["obs_pose"]
        out = []
        for j in points:
            a, b = int(ptr[j]), int(ptr[j + 1])
            v = self.V[j].cpu().numpy()
            Vi = np.linalg.inv(np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]]))
            W = self.W[a:b].cpu().numpy().reshape(-1, 6, 3)
            onodes = [self.P.pose_stride * int(k) for k in obs_pose[a:b].cpu().numpy()]
            out.append(([w @ Vi for w in W], onodes, Vi))
        return out

    def _point_cov(self, Sigma):
        nL = self.P.n_points
        cov = torch.empty((nL, 9), dtype=torch.float64, device=self.P.device)
        if nL:
            _lib.call("vus_ba_point_covariance", self._pp(), ctypes.addressof(self.P.c_tiles), _lib.ptr(self.W),
                      _lib.ptr(self.Vinv), _lib.ptr(Sigma), self.P.band, _lib.ptr(cov), _lib.current_stream_ptr())
        return cov.reshape(nL, 3, 3)

    def _pose_blocks(self, Sigma, nodes):
        return Sigma[nodes, 0].reshape(-1, 6, 6)

    def marginals(self, poses, points, points_cov=True) -> BAMarginals:
        """Marginal covariances at (poses, points) -- which need not be an optimum -- with the robust weights of that
        point and no damping: S at lambda = 0, its one-sided factor, the selected inversion of the band and the landmark
        covariances.  Raises IndeterminantSystem when the information matrix is not positive definite.  Reuses the
        solver's workspace; a later optimize() is unaffected."""
        values, Sigma, nodes, pc = self._marginal_parts((poses, points), points_cov)
        return BAMarginals(self, values, Sigma, self._pose_blocks(Sigma, nodes), pc)

    def _marginal_parts(self, values, points_cov, correct=None):
        """What every marginals() starts from: (`values` as contiguous float64, the band Sigma of the camera-side
        covariance, the pose nodes, the landmark covariances or None).  `correct(Sigma)`, if given, amends the band in
        place before the landmark covariances are formed from it."""
        self._refuse_long("marginals()")
        values = tuple(x.to(torch.float64).contiguous() for x in values)
        self._marginal_factor(values)
        Sigma = self._selinv()
        if correct is not None:
            correct(Sigma)
        nodes = torch.arange(self.P.n_poses, device=self.P.device) * self.P.pose_stride
        return values, Sigma, nodes, self._point_cov(Sigma) if points_cov else None

    def _exact_covariance_columns(self, values, nodes, U=None, Snb=None):
        """The joint covariance of `nodes` from exact columns of S^-1: vus_ba_band_solve_multi with at most 8 unit
        right-hand sides per call, each after a fresh lambda = 0 Schur step (the solve factorises Sband in place)."""
        self._refuse_long("exact covariance columns")
        nN = self.P.n_nodes
        cols = [6 * q + c for q in nodes for c in range(6)]
        got = np.zeros((len(cols), 6 * nN))
        p = _lib.ptr
        self._linearize_all(values)
        for c0 in range(0, len(cols), 8):
            chunk = cols[c0:c0 + 8]
            while True:
                self._assemble_zero()
                rhs = torch.zeros((len(chunk), 6 * nN), dtype=torch.float64, device=self.P.device)
                rhs[torch.arange(len(chunk)), torch.tensor(chunk)] = 1.0
                _lib.call("vus_ba_band_solve_multi", p(self.Sband), nN, self.P.band, p(rhs), len(chunk), p(self.status),
                          _lib.current_stream_ptr())
                if not self._factor_status():
                    break
            got[c0:c0 + len(chunk)] = rhs.cpu().numpy()
        J = got[:, cols].T
        if U is not None:           # + U_i Sc^-1 U_k^T = -Sigma_nb(i) U_k^T
            Ui = U.cpu().numpy()[:, cols].T                                   # [6m, 6]
            nb = Snb[torch.tensor(nodes, dtype=torch.int64, device=Snb.device)].cpu().numpy().reshape(-1, 6)
            J = J - nb @ Ui.T
        return 0.5 * (J + J.T)

    def _linearize_all(self, values):
        self._lm_linearize(values)
        self._check_points()

    def _assemble_zero(self):
        self._assemble(0.0)

    # -- Levenberg-Marquardt ----------------------------------------------------------------------
    # The stages of one LM iteration over a tuple of state tensors (poses first, points last): the stereo step, then
    # each term of self._terms (the order and what depends on it: __init__).
    _NEW_STATE = ("new_poses", "new_points")      # the buffers a trial writes, one per state tensor

    def _lm_error(self, state) -> float:
        return sum((term.error(state) for term in self._terms), self.error(state[0], state[-1]))

    def _lm_linearize(self, state):
        self.linearize(state[0], state[-1])
        for term in self._terms:
            term.linearize(state)

    def _assemble(self, lam):
        self.schur(lam)
        for term in self._terms:
            term.assemble(lam)

    def _solve(self, lam):
        self.band_solve()
        self._closure_correct(self.dp, 1)

    def _lm_solve(self, lam):
        self._assemble(lam)
        self._solve(lam)
        self.backsub()

    def _lm_eval(self, state):
        """Evaluate the trial step; (status, [linearised error at 0, at the step, new error]) of the whole graph, every
        term's scalars included, from ONE blocking read of the trial record."""
        self.eval_step(state[0], state[-1])
        for term in self._terms:
            term.eval_step(state)
        rec = self._trial.cpu()
        errors = self._trial_errors(rec)
        if self.C is not None:      # max_i C_ii of this trial's capacitance matrix (NaN counts as too large)
            v = float(rec[self._clo_at + 3])
            self._closure_max_diag = max(self._closure_max_diag, v if v == v else math.inf)
            self._closure_loss_trials += int(not v <= self.CLOSURE_MAX_DIAG)
        return int(rec[4:5].view(torch.int32)[0]), errors

    def _lm_swap(self, state):
        """Accept the trial: its buffers become the state, the old state tensors the next trial's buffers."""
        new = tuple(getattr(self, n) for n in self._NEW_STATE)
        for n, old in zip(self._NEW_STATE, state):
            setattr(self, n, old)
        return new

    def optimize(self, poses: torch.Tensor, points: torch.Tensor, params: Optional[LMParams] = None,
                 aux=None):
        """poses [nP,12], points [nL,3] float64 on the GPU; returns optimised copies and an LMReport.
        `aux` (optional) carries host-side variables that decouple from the camera system (vector
        variables with only a prior factor): .error(), .try_lambda(lam) -> (lin, new), .accept()."""
        prm = params or LMParams()
        if prm.diagonalDamping:
            raise NotImplementedError("diagonalDamping=True is not implemented (gtsam default is False)")
        if not prm.useFixedLambdaFactor:
            raise NotImplementedError("useFixedLambdaFactor=False is not implemented (gtsam default is True)")
        state, rep = self._levenberg_marquardt((poses, points), prm, aux)
        return (*state, rep)

    def _levenberg_marquardt(self, state, prm, aux=None):
        """GTSAM's iterate / tryLambda / checkConvergence over copies of `state`; returns (state, LMReport)."""
        state = tuple(x.to(torch.float64).contiguous().clone() for x in state)
        rep = LMReport(setup_seconds=self.P.setup_seconds, long_closures=self.C.n if self.C is not None else 0)
        self._closure_loss_trials, self._closure_max_diag = 0, 0.0
        torch.cuda.synchronize(self.P.device)
        t0 = time.perf_counter()
        lam = prm.lambdaInitial
        current = self._lm_error(state) + (aux.error() if aux else 0.0)
        rep.initial_error = current
        if current <= prm.errorTol or prm.maxIterations <= 0:     # gtsam's defaultOptimize: before the first iterate()
            rep.status, rep.final_error, rep.final_lambda = (0 if current <= prm.errorTol else 1), current, lam
            return state, rep
        while rep.iterations < prm.maxIterations:
            self._lm_linearize(state)                             # iterate(): linearise once
            new_error, stop_search, accepted, lin0 = current, False, False, None
            while True:                                           # tryLambda
                self._lm_solve(lam)
                status, sc = self._lm_eval(state)
                if status < 0:
                    if self._window_expired(status):              # the band is spoilt: redo this trial launch by launch
                        continue
                    raise RuntimeError("vus_ba_band_solve: the cooperative back-substitution timed out (status %d)" % status)
                rep.tries += 1
                a_lin, a_new = aux.try_lambda(lam) if aux else (0.0, 0.0)
                if lin0 is None:
                    lin0 = sc[0] + (aux.error() if aux else 0.0)
                success = False
                lin1, new1 = sc[1] + a_lin, sc[2] + a_new
                if status == 0 and math.isfinite(lin1) and math.isfinite(new1):
                    lin_change = lin0 - lin1
                    if lin_change >= 0.0:
                        cost_change = current - new1
                        if lin_change > 2.220446049250313e-16 * lin0:
                            success = cost_change / lin_change > prm.minModelFidelity
                        if abs(cost_change) < prm.relativeErrorTol * current:
                            stop_search = True
                        if success:
                            state = self._lm_swap(state)
                            new_error = new1
                            if aux:
                                aux.accept()
                if success:
                    lam = max(prm.lambdaLowerBound, lam / prm.lambdaFactor)
                    accepted = True
                    break
                if stop_search:
                    break
                lam *= prm.lambdaFactor
                if lam >= prm.lambdaUpperBound:
                    rep.status = 2
                    break
            rep.err_hist.append(new_error)
            rep.lambda_hist.append(lam)
            rep.outer += 1
            rep.iterations += int(accepted)
            if new_error <= prm.errorTol:
                converged = True
            else:
                abs_dec = current - new_error
                converged = (abs_dec / current <= prm.relativeErrorTol) or (abs_dec <= prm.absoluteErrorTol)
            current = new_error
            if rep.status == 2 or converged or not math.isfinite(current):
                if converged and rep.status != 2:
                    rep.status = 0
                break
        torch.cuda.synchronize(self.P.device)
        rep.seconds = time.perf_counter() - t0
        rep.final_error, rep.final_lambda = current, lam
        rep.closure_loss_trials, rep.closure_max_diag = self._closure_loss_trials, self._closure_max_diag
        return state, rep


# ---------------------------------------------------------------------------------------------
# graphs with inertial / velocity factors, in two node layouts: one shared IMU bias
# (vus_nav_*, pose_stride 2) and one bias per keyframe (include/vus_nav_bias.h vus_navb_*, pose_stride 3)
class _InertialFactors:
    """The device tensors both factor structs share (IMU, DVL, velocity priors) and the _CNav prefix of the struct."""
    _IMU_REFUSAL = "ImuFactor between non-consecutive poses is not supported"

    def __init__(self, gravity, imu, dvl, vprior, device):
        self.dev = torch.device(device)
        z = []
        self.imu_i, self.imu_j = self._pair(imu, self._IMU_REFUSAL)
        self.imu_pim = _upload(imu[2] if imu else z, self.dev, torch.float64, (-1, 148))
        self.imu_W = _upload(imu[3] if imu else z, self.dev, torch.float64, (-1, 81))
        self.dvl_pose = _upload(dvl[0] if dvl else z, self.dev, torch.int32, (-1,))
        self.dvl_meas = _upload(dvl[1] if dvl else z, self.dev, torch.float64, (-1, 3))
        self.dvl_w = self._inv(dvl[2] if dvl else z, (-1,))
        self.vp_idx = _upload(vprior[0] if vprior else z, self.dev, torch.int32, (-1,))
        self.vp_v = _upload(vprior[1] if vprior else z, self.dev, torch.float64, (-1, 3))
        self.vp_w = self._inv(vprior[2] if vprior else z, (-1, 3))
        self._c_prefix = (self.imu_i.numel(), self._pp(self.imu_i), self._pp(self.imu_j), self._pp(self.imu_pim),
                          self._pp(self.imu_W), (c_double * 3)(*[float(g) for g in gravity]), self.dvl_pose.numel(),
                          self._pp(self.dvl_pose), self._pp(self.dvl_meas), self._pp(self.dvl_w), self.vp_idx.numel(),
                          self._pp(self.vp_idx), self._pp(self.vp_v), self._pp(self.vp_w))
        self.n_factors = self.imu_i.numel() + self.dvl_pose.numel() + self.vp_idx.numel()

    def _inv(self, sigma, shape):
        """1/sigma on the device: the whitening weight of a diagonal noise model"""
        return (1.0 / _upload(sigma, self.dev, torch.float64, shape)).contiguous()

    def _pair(self, fac, refusal):
        """(i, j) index tensors of a factor that must join consecutive variables (j = i + 1)"""
        i = _upload(fac[0] if fac else [], self.dev, torch.int32, (-1,))
        j = _upload(fac[1] if fac else [], self.dev, torch.int32, (-1,))
        if i.numel() and bool((j - i != 1).any()):
            raise NotImplementedError(refusal)
        return i, j

    @staticmethod
    def _pp(x):
        return _lib.ptr(x) if x.numel() else None

    def addr(self):
        return ctypes.addressof(self.c)


class NavFactors(_InertialFactors):
    """Device-resident vus_nav_factors.  imu = (i, j, pim [n,148], W [n,81]); dvl = (pose, meas [n,3], sigma [n]);
    vprior = (idx, v [n,3], sigmas [n,3]).  ImuFactors must join consecutive poses (j = i + 1)."""
    _IMU_REFUSAL = "ImuFactor between non-consecutive poses is not supported (batch.py:238 joins i-1 and i)"

    def __init__(self, gravity, imu=None, dvl=None, vprior=None, device="cuda:0"):
        super().__init__(gravity, imu, dvl, vprior, device)
        self.c = _CNav(*self._c_prefix)


class NavBiasFactors(_InertialFactors):
    """Device-resident vus_navb_factors.  imu, dvl, vprior as NavFactors (ImuFactor f uses bias B(imu_i[f]));
    bbetween = (i, j, meas [n,6], sigmas [n,6]) for BetweenFactorConstantBias(B(i), B(j = i + 1)), bprior = (idx,
    mean [n,6], sigmas [n,6]) for PriorFactorConstantBias.  Diagonal noise models; 6-vectors in the order (acc, gyro)."""

    def __init__(self, gravity, imu=None, dvl=None, vprior=None, bbetween=None, bprior=None, device="cuda:0"):
        super().__init__(gravity, imu, dvl, vprior, device)
        z = []
        self.bb_i, self.bb_j = self._pair(bbetween, "BetweenFactorConstantBias between non-consecutive biases is not "
                                                    "supported")
        self.bb_meas = _upload(bbetween[2] if bbetween else z, self.dev, torch.float64, (-1, 6))
        self.bb_w = self._inv(bbetween[3] if bbetween else z, (-1, 6))
        self.bp_idx = _upload(bprior[0] if bprior else z, self.dev, torch.int32, (-1,))
        self.bp_mean = _upload(bprior[1] if bprior else z, self.dev, torch.float64, (-1, 6))
        self.bp_w = self._inv(bprior[2] if bprior else z, (-1, 6))
        pp = self._pp
        self.c = _CNavBias(*self._c_prefix, self.bb_i.numel(), pp(self.bb_i), pp(self.bb_j), pp(self.bb_meas),
                           pp(self.bb_w), self.bp_idx.numel(), pp(self.bp_idx), pp(self.bp_mean), pp(self.bp_w))

    def unconstrained_biases(self, n_poses, combined=None):
        """Biases with neither a prior, a between-factor nor a CombinedImuFactor of `combined` (whose rows 9..14 tie B(i) to
        B(i+1) as a between-factor does): their information comes from ImuFactors alone, if any."""
        seen = np.zeros(n_poses, bool)
        bb_i, bp_idx = self.bb_i.cpu().numpy().astype(np.int64), self.bp_idx.cpu().numpy().astype(np.int64)
        ci = combined.host["i"] if combined is not None else np.zeros(0, np.int64)
        for a in (bb_i, bb_i + 1, bp_idx, ci, ci + 1):
            seen[a[(a >= 0) & (a < n_poses)]] = True
        return np.nonzero(~seen)[0]


class CombinedImuFactors:
    """Device-resident vus_cimu_factors (include/vus_combined_imu.h): CombinedImuFactor(X(i), V(i), X(i+1), V(i+1), B(i),
    B(i+1)) for the keyframes `i` [n], with pim [n, 148] the preintegration records and W [n, 225] the 15 x 15 whitening
    matrices (gtsam/imu.py CombinedPreintegrator.packed() / .whitening()).  `j` (None: i + 1) may name the later keyframes;
    anything but i + 1 is refused.  An add-on to NavBiasFactors: NavBiasBASolver(problem, nav, combined=...)."""

    def __init__(self, gravity, i, pim, W, device="cuda:0", j=None):
        i = np.asarray(i, np.int64).reshape(-1)
        j = i + 1 if j is None else np.asarray(j, np.int64).reshape(-1)
        pim = np.asarray(pim, np.float64).reshape(-1, 148)
        W = np.asarray(W, np.float64).reshape(-1, 225)
        n = len(i)
        if n == 0 or not (len(j) == len(pim) == len(W) == n):
            raise ValueError(f"combined IMU factors: {len(i)} / {len(j)} keyframes, {len(pim)} records, {len(W)} whitening matrices")
        if (j != i + 1).any():
            f = int(np.nonzero(j != i + 1)[0][0])
            raise NotImplementedError(f"CombinedImuFactor {f} joins keyframes {int(i[f])} and {int(j[f])}: a CombinedImuFactor "
                                      "between non-consecutive keyframes is not supported")
        if (i < 0).any():
            raise ValueError("combined IMU factors: a negative keyframe index")
        if not (np.isfinite(pim).all() and np.isfinite(W).all()):
            raise ValueError("combined IMU factors: pim and W must be finite")
        self.n = n
        self.host = dict(i=i, pim=pim, W=W)
        dev = torch.device(device)
        self.i, self.j = _upload(i, dev, torch.int32), _upload(j, dev, torch.int32)
        self.pim, self.W = _upload(pim, dev, torch.float64), _upload(W, dev, torch.float64)
        p = _lib.ptr
        self.c = _CCombinedImu(n, p(self.i), p(self.j), p(self.pim), p(self.W), (c_double * 3)(*[float(g) for g in gravity]))

    def addr(self):
        return ctypes.addressof(self.c)

    def _fits(self, problem):
        """Refuse a StereoBAProblem this set was not built for (the solver asks before it uses the set)."""
        if problem.pose_stride != 3:
            raise ValueError(f"CombinedImuFactors serve pose_stride 3 only (the per-keyframe-bias layout of NavBiasBASolver), "
                             f"the problem has pose_stride {problem.pose_stride}")
        if int(self.host["i"].max()) + 1 >= problem.n_poses:
            raise ValueError(f"CombinedImuFactors: keyframe {int(self.host['i'].max()) + 1} outside the problem's "
                             f"{problem.n_poses} poses")
        if problem.band < min(5, problem.n_nodes - 1):
            raise ValueError(f"a CombinedImuFactor couples nodes 5 apart, more than the problem's band of {problem.band} nodes: "
                             "build the StereoBAProblem with combined_imu=True")


class _InertialBASolver(StereoBASolver):
    """LM over poses, velocities, IMU biases and landmarks: the stereo solver plus the inertial factors of one node
    layout.  A subclass names its pose_stride, Snav's block diagonals, its entry points (`_ABI`) and its bias shape."""
    POSE_STRIDE = SDIAG = None
    _ABI = None
    _NEW_STATE = ("new_poses", "new_vels", "new_bias", "new_points")     # state = (poses, vels, bias, points)

    def __init__(self, problem: StereoBAProblem, nav, bias_rows, between=None, point_priors=None, pose_meas=None,
                 window_prior=None, more_inertial=()):
        if window_prior is not None and not isinstance(window_prior, NavWindowPrior):
            raise NotImplementedError(f"a dense prior over a pose window (ba.WindowPrior) is not supported by {type(self).__name__}: "
                                      "the family serves the pose-only layout (StereoBASolver)")
        if window_prior is not None and self.POSE_STRIDE != 3:
            raise NotImplementedError(f"a dense prior over an inertial window (ba.NavWindowPrior) is not supported by "
                                      f"{type(self).__name__}: the family serves the per-keyframe-bias layout (NavBiasBASolver)")
        if problem.pose_stride != self.POSE_STRIDE:
            raise ValueError(f"{type(self).__name__} needs a StereoBAProblem built with pose_stride={self.POSE_STRIDE}")
        nav3 = lambda stage: lambda s: stage(*s[:3])          # state = (poses, vels, bias, points)

        def nav_eval(s):        # the nav window prior's after the inertial one, which writes new_vels and new_bias
            self.nav_eval_step(*s[:3])
            self.nav_window_prior_eval_step(*s[:3])
        super().__init__(problem, between, point_priors, inertial=[
            ("nav_scal", nav3(self.nav_error), nav3(self.nav_linearize), self.nav_assemble, nav_eval), *more_inertial],
            pose_meas=pose_meas, window_prior=window_prior)
        self.N = nav
        dev, nP, nN = problem.device, problem.n_poses, problem.n_nodes
        f64 = dict(dtype=torch.float64, device=dev)
        self.Snav = torch.empty((nN, self.SDIAG, 36), **f64)
        self.gnav = torch.empty((nN, 6), **f64)
        self.new_vels = torch.empty((nP, 3), **f64)
        self.new_bias = torch.empty((6,) if bias_rows is None else (bias_rows, 6), **f64)
        self.nav_work = torch.empty((int(getattr(_lib.load(), self._ABI + "_work_doubles")(nav.addr())),), **f64)

    def nav_error(self, poses, vels, bias) -> float:
        p = _lib.ptr
        _lib.call(self._ABI + "_error", self.N.addr(), self.P.n_poses, p(poses), p(vels), p(bias), p(self.nav_scal),
                  p(self.nav_work), _lib.current_stream_ptr())
        return float(self.nav_scal[0].item())

    def optimize(self, poses, vels, bias, points, params: Optional[LMParams] = None):
        """Returns (poses, vels, bias, points, LMReport); inputs untouched."""
        prm = params or LMParams()
        if prm.diagonalDamping or not prm.useFixedLambdaFactor:
            raise NotImplementedError("only the gtsam defaults diagonalDamping=False, useFixedLambdaFactor=True")
        state, rep = self._levenberg_marquardt((poses, vels, bias, points), prm)
        return (*state, rep)


class NavBASolver(_InertialBASolver):
    """LM over poses, velocities, one shared IMU bias and landmarks.  The problem must have been built with
    pose_stride=2 (velocity nodes interleaved); the bias is a 6-wide border eliminated after a
    7-right-hand-side band solve."""
    POSE_STRIDE, SDIAG, _ABI = 2, 4, "vus_nav"

    def __init__(self, problem: StereoBAProblem, nav: NavFactors, between: Optional[BetweenFactors] = None,
                 point_priors: Optional[PointPriors] = None, pose_meas: Optional[PoseMeasurements] = None, window_prior=None,
                 combined=None):
        if combined is not None:
            raise NotImplementedError("CombinedImuFactor (ba.CombinedImuFactors) is not supported by NavBASolver: it ties B(i) to "
                                      "B(i+1), which the shared-bias layout does not have; use NavBiasBASolver (pose_stride 3)")
        super().__init__(problem, nav, None, between, point_priors, pose_meas, window_prior)
        self.band_rhs = 7
        self._alloc_band_work()
        nN = problem.n_nodes
        f64 = dict(dtype=torch.float64, device=problem.device)
        self.Scb = torch.empty((nN, 36), **f64)
        self.Sbb = torch.empty((36,), **f64)
        self.gb = torch.empty((6,), **f64)
        self.rhs = torch.empty((7, nN * 6), **f64)
        self.db = torch.empty((6,), **f64)

    def nav_linearize(self, poses, vels, bias):
        p = _lib.ptr
        _lib.call("vus_nav_linearize", self.N.addr(), self.P.n_poses, p(poses), p(vels), p(bias), p(self.Snav),
                  p(self.Scb), p(self.Sbb), p(self.gnav), p(self.gb), p(self.nav_scal), p(self.nav_work),
                  _lib.current_stream_ptr())

    def nav_assemble(self, lam):
        p = _lib.ptr
        _lib.call("vus_nav_assemble", self.P.n_nodes, self.P.band, float(lam), p(self.Snav), p(self.Scb), p(self.gnav),
                  p(self.Sband), p(self.gs), p(self.rhs), _lib.current_stream_ptr())

    def nav_solve(self, lam):
        p = _lib.ptr
        st = _lib.current_stream_ptr()
        if self.use_split:
            _lib.call("vus_ba_band_solve_multi_split", p(self.Sband), self.P.n_nodes, self.P.band, p(self.rhs), 7,
                      p(self.status), p(self.band_work), st)
        else:
            _lib.call("vus_ba_band_solve_multi", p(self.Sband), self.P.n_nodes, self.P.band, p(self.rhs), 7, p(self.status), st)
        self._closure_correct(self.rhs, 7)          # all 7 columns, before the bias border is eliminated with them
        _lib.call("vus_nav_border_solve", self.P.n_nodes, p(self.rhs), p(self.Scb), p(self.Sbb), p(self.gb), float(lam),
                  p(self.dp), p(self.db), st)

    _solve = nav_solve

    def nav_eval_step(self, poses, vels, bias):
        p = _lib.ptr
        _lib.call("vus_nav_eval_step", self.N.addr(), self.P.n_poses, p(poses), p(vels), p(bias), p(self.dp), p(self.db),
                  p(self.new_poses), p(self.new_vels), p(self.new_bias), p(self.nav_scal[1:]), p(self.nav_work),
                  _lib.current_stream_ptr())

    def _factor_zero(self):
        p = _lib.ptr
        _lib.call("vus_ba_band_solve_multi", p(self.Sband), self.P.n_nodes, self.P.band, p(self.rhs), 7, p(self.status),
                  _lib.current_stream_ptr())

    def marginals(self, poses, vels, bias, points, points_cov=True) -> BAMarginals:
        """StereoBASolver.marginals for the whole graph: the camera-side band of A^-1 (poses and velocity nodes, one-sided
        7-right-hand-side solve at lambda = 0), then the shared-bias border (vus_nav_border_covariance), then the landmark
        covariances from the corrected band."""
        nN, nP = self.P.n_nodes, self.P.n_poses
        p = _lib.ptr
        f64 = dict(dtype=torch.float64, device=self.P.device)
        Snb, Sbb, ok = torch.empty((nN, 36), **f64), torch.empty((36,), **f64), torch.empty((1,), **f64)

        def border(Sigma):
            _lib.call("vus_nav_border_covariance", nN, self.P.band, p(self.rhs), p(self.Scb), p(self.Sbb), p(Sigma), p(Snb),
                      p(Sbb), p(ok), _lib.current_stream_ptr())
            if float(ok.item()) != 1.0:
                raise IndeterminantSystem("bias", 0)
        values, Sigma, pose_nodes, pc = self._marginal_parts((poses, vels, bias, points), points_cov, border)
        U = self.rhs[1:7].clone()
        vel = Sigma[pose_nodes + 1, 0].reshape(nP, 6, 6)[:, :3, :3]
        return BAMarginals(self, values, Sigma, self._pose_blocks(Sigma, pose_nodes), pc, U=U, vel_cov=vel,
                           bias_cov=Sbb.reshape(6, 6), node_bias_cov=Snb.reshape(nN, 6, 6))


class NavBiasBASolver(_InertialBASolver):
    """LM over poses, velocities, ONE IMU BIAS PER KEYFRAME and landmarks (GTSAM's usual visual-inertial graph).  The
    problem must have been built with pose_stride=3: node 3i = X(i), 3i+1 = V(i) padded to 6, 3i+2 = B(i).  There is no
    border; every lambda trial is one single-right-hand-side band solve (two-sided on long graphs).  optimize() is the
    common inertial loop, with `bias` the [n_poses, 6] per-keyframe biases.
    `combined`: CombinedImuFactors (include/vus_combined_imu.h) on some or all intervals, one more stage after the inertial
    one; the problem is then built with combined_imu=True.  Without it nothing this solver launches changes."""
    POSE_STRIDE, SDIAG, _ABI = 3, 5, "vus_navb"

    def __init__(self, problem: StereoBAProblem, nav: NavBiasFactors, between: Optional[BetweenFactors] = None,
                 point_priors: Optional[PointPriors] = None, pose_meas: Optional[PoseMeasurements] = None, window_prior=None,
                 combined: Optional[CombinedImuFactors] = None):
        self.CI = combined
        more = ()
        if combined is not None:
            if window_prior is not None:
                raise NotImplementedError("CombinedImuFactor (ba.CombinedImuFactors) together with a dense prior over an inertial "
                                          "window (ba.NavWindowPrior) is not supported")
            combined._fits(problem)
            nav3 = lambda stage: lambda s: stage(*s[:3])
            more = [("cimu_scal", nav3(self.cimu_error), nav3(self.cimu_linearize), lambda lam: self.cimu_assemble(),
                     nav3(self.cimu_eval_step))]
        super().__init__(problem, nav, problem.n_poses, between, point_priors, pose_meas, window_prior, more_inertial=more)
        if combined is not None:
            f64 = dict(dtype=torch.float64, device=problem.device)
            self.Scimu = torch.empty((problem.n_nodes, 6, 36), **f64)
            self.gcimu = torch.empty((problem.n_nodes, 6), **f64)
            self.cimu_err = torch.empty((1,), **f64)
            self.cimu_work = torch.empty((int(_lib.load().vus_cimu_work_doubles(combined.addr())),), **f64)

    # The CombinedImuFactors (include/vus_combined_imu.h): the stages of the term `cimu_scal`, present only with `combined`.
    def cimu_error(self, poses, vels, biases) -> float:
        """Error of the CombinedImuFactors at (poses, vels, biases); 0.0 without them."""
        if self.CI is None:
            return 0.0
        p = _lib.ptr
        _lib.call("vus_cimu_error", self.CI.addr(), self.P.n_poses, p(poses), p(vels), p(biases), p(self.cimu_err),
                  p(self.cimu_work), _lib.current_stream_ptr())
        return float(self.cimu_err[0].item())

    def cimu_linearize(self, poses, vels, biases):
        """Scimu, gcimu = the factors' blocks and gradient, cimu_scal[0] = their error."""
        p = _lib.ptr
        _lib.call("vus_cimu_linearize", self.CI.addr(), self.P.n_poses, p(poses), p(vels), p(biases), p(self.Scimu),
                  p(self.gcimu), p(self.cimu_scal), p(self.cimu_work), _lib.current_stream_ptr())

    def cimu_assemble(self):
        """Sband += Scimu, gs += gcimu: after nav_assemble(), which damps the velocity and bias nodes."""
        p = _lib.ptr
        _lib.call("vus_cimu_assemble", self.P.n_nodes, self.P.band, p(self.Scimu), p(self.gcimu), p(self.Sband), p(self.gs),
                  _lib.current_stream_ptr())

    def cimu_eval_step(self, poses, vels, biases):
        """cimu_scal[1] = linearised error at the step dp, cimu_scal[2] = error at the new state (after nav_eval_step)."""
        p = _lib.ptr
        _lib.call("vus_cimu_eval_step", self.CI.addr(), self.P.n_poses, p(poses), p(vels), p(biases), p(self.dp),
                  p(self.new_poses), p(self.new_vels), p(self.new_bias), p(self.cimu_scal[1:]), p(self.cimu_work),
                  _lib.current_stream_ptr())

    def nav_linearize(self, poses, vels, biases):
        p = _lib.ptr
        _lib.call("vus_navb_linearize", self.N.addr(), self.P.n_poses, p(poses), p(vels), p(biases), p(self.Snav),
                  p(self.gnav), p(self.nav_scal), p(self.nav_work), _lib.current_stream_ptr())

    def nav_assemble(self, lam):
        p = _lib.ptr
        _lib.call("vus_navb_assemble", self.P.n_nodes, self.P.band, float(lam), p(self.Snav), p(self.gnav),
                  p(self.Sband), p(self.gs), _lib.current_stream_ptr())

    def nav_solve(self, lam):
        self.band_solve()           # no border: the same as the stereo solver's _solve

    def nav_eval_step(self, poses, vels, biases):
        p = _lib.ptr
        _lib.call("vus_navb_eval_step", self.N.addr(), self.P.n_poses, p(poses), p(vels), p(biases), p(self.dp),
                  p(self.new_poses), p(self.new_vels), p(self.new_bias), p(self.nav_scal[1:]), p(self.nav_work),
                  _lib.current_stream_ptr())

    def _refuse_free_biases(self, upto):
        """IndeterminantSystem("bias", i) for the first bias B(i), i < upto, with neither a prior, a between-factor nor a place
        in the nav window prior.  A bias that is singular all the same is caught by the factor's pivot test, as a node."""
        free = self.N.unconstrained_biases(self.P.n_poses, self.CI)
        if self.NWP is not None:
            free = free[(free < self.NWP.first) | (free >= self.NWP.first + self.NWP.m)]
        free = free[free < upto]
        if len(free):
            raise IndeterminantSystem("bias", int(free[0]))

    def marginalize_head(self, poses, vels, biases, points, n_drop) -> NavWindowPrior:
        """Eliminate every landmark and the first `n_drop` KEYFRAMES -- pose, velocity and bias -- of THIS solver's problem at
        (poses, vels, biases, points) and return the Gaussian prior that leaves on the remaining keyframes: a NavWindowPrior
        with first = 0, m = n_poses - n_drop and the linearisation point (poses, vels, biases)[n_drop:], for a problem of
        those m keyframes.  The linear system is the one marginals() uses -- no damping, the robust weights of that point,
        the velocity padding at unit diagonal and zero right-hand side; vus_ba_band_marginalize eliminates 3 n_drop nodes,
        the padding rows of what it returns are identity rows that vus_nav_window_prior_compact leaves out.  c = the linear
        error at a zero step of all terms (the inertial ones and a nav window prior of this solver included)
        - 0.5 g_M^T S_MM^-1 g_M - 0.5 sum_l gl_l^T V_l^-1 gl_l.  Raises IndeterminantSystem("bias", i) for a dropped bias
        without a prior, a between-factor or a place in this solver's prior, ("point", j) / ("node", i) where the eliminated
        part is not positive definite."""
        self._refuse_long("marginalize_head()")
        if self.CI is not None:
            raise NotImplementedError("marginalize_head() with CombinedImuFactors (ba.CombinedImuFactors) is not supported")
        nP, nN, B, k = self.P.n_poses, self.P.n_nodes, self.P.band, int(n_drop)
        if not 1 <= k < nP:
            raise ValueError(f"marginalize_head: n_drop={k} outside [1, n_poses={nP})")
        if 3 * (nP - k) - 1 > B:
            raise ValueError(f"marginalize_head: the {nP - k} remaining keyframes ({3 * (nP - k)} nodes) do not fit the band of "
                             f"{B} nodes: build the StereoBAProblem with between_span={nP - k}")
        self._refuse_free_biases(k)
        values = tuple(x.to(torch.float64).contiguous() for x in (poses, vels, biases, points))
        self._linearize_all(values)
        self._assemble_zero()
        w = nP - k
        f64 = dict(dtype=torch.float64, device=self.P.device)
        H18, g18, quad = torch.empty((18 * w, 18 * w), **f64), torch.empty((18 * w,), **f64), torch.empty((1,), **f64)
        H, g = torch.empty((15 * w, 15 * w), **f64), torch.empty((15 * w,), **f64)
        status = torch.empty((1,), dtype=torch.int32, device=self.P.device)
        work = torch.empty((int(_lib.load().vus_ba_band_marginalize_work_doubles(nN, B, 3 * k)),), **f64)
        p, st = _lib.ptr, _lib.current_stream_ptr()
        _lib.call("vus_ba_band_marginalize", p(self.Sband), nN, B, p(self.gs), 3 * k, p(H18), p(g18), p(quad), p(status), p(work), st)
        _lib.call("vus_nav_window_prior_compact", p(H18), p(g18), w, p(H), p(g), st)
        bad = int(status.item())
        if bad > 0:
            raise IndeterminantSystem("node", (bad - 1) // 6)
        lin0 = self._trial_errors(self._trial.cpu())[0]
        land = 0.0
        if self.P.n_points:     # gl^T V^-1 gl per landmark; Vinv is what the Schur step at lambda = 0 left (upper triangle)
            vi, gl = self.Vinv, self.gl
            x, y, z = gl[:, 0], gl[:, 1], gl[:, 2]
            land = float((vi[:, 0] * x * x + vi[:, 3] * y * y + vi[:, 5] * z * z
                          + 2.0 * (vi[:, 1] * x * y + vi[:, 2] * x * z + vi[:, 4] * y * z)).sum().item())
        c = lin0 - 0.5 * float(quad.item()) - 0.5 * land
        return NavWindowPrior(0, values[0][k:], values[1][k:], values[2][k:], H, g, c, w, device=self.P.device)

    def marginals(self, poses, vels, biases, points, points_cov=True) -> BAMarginals:
        """Marginal covariances at (poses, vels, biases, points): the one-sided factor of the whole camera-side system at
        lambda = 0 and its selected inversion -- no border step, every bias is a band node.  The BAMarginals carries
        vel_cov [n, 3, 3] and biases_cov [n, 6, 6] (B(i) is node 3i + 2, for joint()).  Raises IndeterminantSystem("bias",
        i) for a bias B(i) with neither a prior, a between-factor nor a place in the solver's NavWindowPrior."""
        self._refuse_free_biases(self.P.n_poses)
        values, Sigma, nodes, pc = self._marginal_parts((poses, vels, biases, points), points_cov)
        nP = self.P.n_poses
        return BAMarginals(self, values, Sigma, self._pose_blocks(Sigma, nodes), pc,
                           vel_cov=Sigma[nodes + 1, 0].reshape(nP, 6, 6)[:, :3, :3],
                           biases_cov=Sigma[nodes + 2, 0].reshape(nP, 6, 6))
