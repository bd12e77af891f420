"""Numpy reference of the partial absolute measurements on poses (include/vus_pose_meas.h) for the tests: the two
residual kinds

    POSITION   r = W (t + R a - m),    J = W [ -R [a]x , R ]
    ROTATION   r = W Log(Rm^T R),      J = W [ I3 , 0 ]            (the derivative of Log is not applied)

with each factor's own robust model (Block reweighting: r and J scaled by sqrt(w(|r|)), linear slots 0.5 sum w |b + J d|^2,
nonlinear slots sum rho), and point_prior_ref.PointPriorBA with their term added to Hpp / gp, to the error and to the step
evaluation.  The damped solve, the LM and the dense information matrix are inherited unchanged: they read Hpp, gp and the
error scalars only.  This file is the CPU statement of the feature; it also draws the factor sets of the GPU tests."""
import math

import numpy as np

import point_prior_ref
from robust_ref import weight_loss

POSITION, ROTATION = 0, 1


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = skew(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + math.sin(th) / th * K + 2.0 * math.sin(0.5 * th) ** 2 / (th * th) * (K @ K)


def so3_log(R):
    """Log of a rotation matrix, to a few eps at every angle below pi: the angle from atan2(sin, cos); the axis from the
    antisymmetric part, or above 2.4 rad (where that part fades) from the symmetric part, signed by the antisymmetric."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * float(np.linalg.norm(v)), 0.5 * (float(np.trace(R)) - 1.0)
    th = math.atan2(s, c)
    if c > -0.7:
        return v * (0.5 + (th * th) / 12.0 if th < 1e-5 else th / (2.0 * s))
    S = 0.5 * (R + R.T) - c * np.eye(3)               # (1 - cos th) a a^T
    a = S[:, int(np.argmax(np.diag(S)))]
    a = a / np.linalg.norm(a)
    return th * (a if float(v @ a) >= 0.0 else -a)


def raw_factor(kind, m9, T):
    """unwhitened residual r [3] and Jacobian J [3,6] (tangent order (omega, v)) of one factor at the pose T (flat12)"""
    T, m9 = np.asarray(T, np.float64), np.asarray(m9, np.float64)
    R, t = T[:9].reshape(3, 3), T[9:]
    if kind == ROTATION:
        return so3_log(m9.reshape(3, 3).T @ R), np.hstack([np.eye(3), np.zeros((3, 3))])
    m, a = m9[:3], m9[3:6]
    return (t - m) + R @ a, np.hstack([-R @ skew(a), R])


def _wl(kind, k, d2):
    """(w, rho) of the robust table at the squared whitened norm d2 (Gaussian: 1, d2 / 2)."""
    if kind == 0:
        return 1.0, 0.5 * d2
    w, rho = weight_loss(kind, k, np.array([math.sqrt(d2)]))
    return float(w[0]), float(rho[0])


class PoseMeasSet:
    """Host description, in GRAPH order: idx [n] pose indices, kind [n], meas [n,9], sigmas [n,3], losses [(kind, k)]
    (None = all Gaussian)."""

    def __init__(self, idx, kind, meas, sigmas, losses=None):
        self.idx = np.asarray(idx, np.int64).reshape(-1)
        self.kind = np.asarray(kind, np.int64).reshape(-1)
        self.meas = np.asarray(meas, np.float64).reshape(-1, 9)
        self.sigmas = np.asarray(sigmas, np.float64).reshape(-1, 3)
        self.w = 1.0 / self.sigmas
        self.losses = [tuple(x) for x in losses] if losses is not None else [(0, 0.0)] * len(self.idx)
        assert len(self.idx) == len(self.kind) == len(self.meas) == len(self.w) == len(self.losses)

    @property
    def n(self):
        return len(self.idx)

    def csr_order(self):
        """graph position of the factor in every CSR slot (stable sort by pose)"""
        return np.argsort(self.idx, kind="stable")

    def device(self, n_poses, pose_stride=1, device="cuda:0"):
        from visual_underwater_slam_amd.ba import PoseMeasurements
        return PoseMeasurements(self.idx, self.kind, self.meas, self.sigmas, n_poses, pose_stride=pose_stride,
                                loss=list(self.losses), device=device)


def factors(G, poses):
    """Per factor, graph order: (pose, sqrt(w) W r, sqrt(w) W J, w, rho) at poses [nP,12]"""
    out = []
    for f in range(G.n):
        i = int(G.idx[f])
        r, J = raw_factor(int(G.kind[f]), G.meas[f], poses[i])
        d2 = float(((G.w[f] * r) ** 2).sum())
        w, rho = _wl(*G.losses[f], d2)
        s = math.sqrt(w) * G.w[f]
        out.append((i, s * r, s[:, None] * J, w, rho))
    return out


def error(G, poses):
    """sum rho (0.5 |W r|^2 without a robust model)"""
    return float(sum(f[4] for f in factors(G, poses)))


def weights(G, poses):
    """w(d) per factor, graph order"""
    return np.array([f[3] for f in factors(G, poses)])


def blocks(G, poses):
    """(Hpp [nP,36], gp [nP,6], err, factors): sum J^T J and sum J^T r per pose, the linear error at delta = 0"""
    nP = len(poses)
    H, g, e = np.zeros((nP, 6, 6)), np.zeros((nP, 6)), 0.0
    fac = factors(G, poses)
    for i, rw, Jw, _, _ in fac:
        H[i] += Jw.T @ Jw
        g[i] += Jw.T @ rw
        e += 0.5 * float(rw @ rw)
    return H.reshape(nP, 36), g, e, fac


def linear_error(fac, dp):
    """0.5 sum w |b + J d|^2 at the POSE steps dp [nP,6]"""
    e = 0.0
    for i, rw, Jw, _, _ in fac:
        v = rw + Jw @ dp[i]
        e += 0.5 * float(v @ v)
    return e


class PoseMeasBA(point_prior_ref.PointPriorBA):
    """PointPriorBA plus a PoseMeasSet (or None)."""

    def __init__(self, *args, pose_meas=None, **kw):
        super().__init__(*args, **kw)
        self.G = pose_meas if pose_meas is not None else PoseMeasSet([], [], np.zeros((0, 9)), np.ones((0, 3)))

    def pose_meas_error(self, poses):
        return error(self.G, np.asarray(poses, np.float64).reshape(-1, 12))

    def error(self, poses, points):
        return super().error(poses, points) + self.pose_meas_error(poses)

    def linearize(self, poses, points):
        """as PointPriorBA's, with the pose measurements in Hpp, gp and err; `pm_err` keeps their scalar apart"""
        lin = super().linearize(poses, points)
        H, g, e, self._pm_fac = blocks(self.G, np.asarray(poses, np.float64).reshape(-1, 12))
        lin["Hpp"] = lin["Hpp"] + H
        lin["gp"] = lin["gp"] + g
        lin["pm_err"] = e
        lin["err"] = lin["err"] + e
        return lin

    def pose_meas_linear_error(self, dp):
        return linear_error(self._pm_fac, dp)

    def linear_error(self, dp, dl):
        return super().linear_error(dp, dl) + self.pose_meas_linear_error(dp)


# -- factor sets of the GPU tests -------------------------------------------------------------------------------------
def _u(n, salt):
    from visual_underwater_slam_amd import synth
    return synth._hash_uniform(np.arange(n, dtype=np.int64), salt)


def rotation_meas(T, w):
    """the row of a ROTATION factor whose residual at the pose T is w: Rm = R Exp(w)^T"""
    return (np.asarray(T, np.float64)[:9].reshape(3, 3) @ so3_exp(w).T).reshape(9)


def position_meas(T, arm, noise):
    """the row of a POSITION factor with lever arm `arm` whose residual at the pose T is -noise"""
    T = np.asarray(T, np.float64)
    return np.concatenate([T[9:] + T[:9].reshape(3, 3) @ np.asarray(arm, float) + noise, arm, np.zeros(3)])


def fix_set(poses_gt, every_pos=3, every_depth=5, every_rot=7, loss=None, salt=77, displaced=()):
    """The factor set of the solver tests on body poses `poses_gt` [nP,12]: position fixes (every second one with a lever
    arm of up to a metre) on every `every_pos`-th pose, depth-only fixes (sigma = (1e3, 1e3, 0.02)) on every
    `every_depth`-th, rotation fixes on every `every_rot`-th, all measured from the truth with noise of their sigma's
    size, in an order that is NOT sorted by pose.  `loss` = (kind, k) goes on every position fix; the position fixes whose
    position in the returned `pos_slots` is in `displaced` are moved by 5 - 30 m.  Returns (PoseMeasSet, pos_slots = the
    graph positions of the plain position fixes)."""
    nP = len(poses_gt)
    rows = []
    for q, i in enumerate(range(0, nP, every_pos)):
        arm = (np.array([_u(3 * nP, salt + 1)[3 * i + k] for k in range(3)]) - 0.5) * 2.0 / math.sqrt(3.0) if q % 2 else np.zeros(3)
        sig = np.array([0.3, 0.3, 0.5])
        noise = sig * (np.array([_u(3 * nP, salt + 2)[3 * i + k] for k in range(3)]) - 0.5) * 2.0
        rows.append((i, POSITION, position_meas(poses_gt[i], arm, noise), sig, "pos"))
    for i in range(1, nP, every_depth):
        sig = np.array([1e3, 1e3, 0.02])
        noise = sig * (np.array([_u(3 * nP, salt + 3)[3 * i + k] for k in range(3)]) - 0.5) * np.array([0.01, 0.01, 2.0])
        rows.append((i, POSITION, position_meas(poses_gt[i], np.zeros(3), noise), sig, "depth"))
    for i in range(2, nP, every_rot):
        sig = np.array([0.02, 0.03, 0.05])
        w = sig * (np.array([_u(3 * nP, salt + 4)[3 * i + k] for k in range(3)]) - 0.5) * 2.0
        rows.append((i, ROTATION, rotation_meas(poses_gt[i], w), sig, "rot"))
    order = np.argsort(_u(len(rows), salt + 5), kind="stable")          # a fixed shuffle of the graph order
    rows = [rows[int(o)] for o in order]
    pos_slots = [f for f, r in enumerate(rows) if r[4] == "pos"]
    meas = np.array([r[2] for r in rows])
    for q in displaced:
        f = pos_slots[q]
        u = _u(4 * len(rows), salt + 6)[4 * f:4 * f + 4]
        d = u[:3] - 0.5
        meas[f, :3] += (5.0 + 25.0 * u[3]) * d / np.linalg.norm(d)
    lo = (0, 0.0) if loss is None else (int(loss[0]), float(loss[1]))
    losses = [lo if r[4] == "pos" else (0, 0.0) for r in rows]
    return PoseMeasSet([r[0] for r in rows], [r[1] for r in rows], meas, np.array([r[3] for r in rows]), losses), pos_slots

