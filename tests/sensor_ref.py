"""Numpy reference of the stereo factors with a camera-to-body extrinsic (include/vus_sensor.h) for the tests:
robust_ref.RobustBA with every factor evaluated at the CAMERA pose C = X o S (composed in float64) by the CPU oracle's
stereo factor, and its pose Jacobian taken to the body tangent, H1_body = H1_cam Ad(S^-1).  Everything else -- the
robust weights, the linearisation, the step evaluation, the damped solve and the LM -- is inherited unchanged."""
import numpy as np

import robust_ref


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def compose(X, S):
    """X o S for flat12 poses (R row-major, then t)."""
    X, S = np.asarray(X, np.float64), np.asarray(S, np.float64)
    Rb, tb, Rs, ts = X[:9].reshape(3, 3), X[9:], S[:9].reshape(3, 3), S[9:]
    return np.concatenate([(Rb @ Rs).reshape(9), tb + Rb @ ts])


def inverse(S):
    S = np.asarray(S, np.float64)
    R, t = S[:9].reshape(3, 3), S[9:]
    return np.concatenate([R.T.reshape(9), -R.T @ t])


def adjoint_of_inverse(S):
    """Ad(S^-1) for the tangent ordered [omega, v]: [[Rs^T, 0], [-Rs^T [ts]x, Rs^T]]."""
    S = np.asarray(S, np.float64)
    Rs, ts = S[:9].reshape(3, 3), S[9:]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = Rs.T
    Ad[3:, :3] = -Rs.T @ skew(ts)
    return Ad


def extrinsic(optical_axes=True):
    """The extrinsic of the tests: the reference's DELTA translation (batch.py:190-193) with a rotation far from the
    identity -- the body (x forward, y left, z up) -> optical (x right, y down, z forward) axis permutation composed with
    Rot3.Ypr(0.3, -0.2, 0.1) -- so that a transposed Rs cannot pass.  optical_axes=False leaves the permutation out."""
    cy, sy, cp, sp, cr, sr = np.cos(0.3), np.sin(0.3), np.cos(-0.2), np.sin(-0.2), np.cos(0.1), np.sin(0.1)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    optical = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # columns: optical axes in the body frame
    return np.concatenate([((optical if optical_axes else np.eye(3)) @ (Rz @ Ry @ Rx)).reshape(9), [0.05, -0.10, 0.20]])


class SensorBA(robust_ref.RobustBA):
    """RobustBA whose poses are BODY poses; the left camera sits at pose o S."""

    def __init__(self, O, pk, K, sigma, kind, k, S, priors=None):
        super().__init__(O, pk, K, sigma, kind, k, priors)
        self.S = np.asarray(S, np.float64).reshape(12)
        self.Ad = adjoint_of_inverse(self.S)

    def factors(self, poses, points, jac=True):
        """whitened r [n,3], H1 [n,3,6] (body tangent), H2 [n,3,3], L-order"""
        cams = np.stack([compose(p, self.S) for p in np.asarray(poses, np.float64).reshape(-1, 12)])
        r, H1, H2 = super().factors(cams, points, jac)
        return r, H1 @ self.Ad, H2

    def full_hessian(self, poses, points):
        """Dense information matrix of all poses then all landmarks at (poses, points), with the robust weights of that
        point and the priors: [6 nP + 3 nL] square."""
        lin = self.linearize(poses, points)
        nP, nL = self.nP, self.nL
        H = np.zeros((6 * nP + 3 * nL, 6 * nP + 3 * nL))
        iu = np.triu_indices(3)
        for i in range(nP):
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = lin["Hpp"][i].reshape(6, 6)
        for j in range(nL):
            V = np.zeros((3, 3)); V[iu] = lin["V"][j]
            H[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3] = V + np.triu(V, 1).T
        W = lin["W"].reshape(-1, 6, 3)
        for a in range(self.nO):
            i, j = self.op[a], self.ol[a]
            H[6 * i:6 * i + 6, 6 * nP + 3 * j:6 * nP + 3 * j + 3] += W[a]
            H[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * i:6 * i + 6] += W[a].T
        return H


def body_sequence(seq, S):
    """A synth.ba_sequence whose poses are camera poses C, restated with body poses X = C o S^-1 (ground truth and
    initial values); measurements and points stay as they are."""
    Sinv = inverse(S)
    out = dict(seq)
    for key in ("poses_gt", "poses_init"):
        out[key] = np.stack([compose(c, Sinv) for c in seq[key]])
    return out
