"""Numpy reference of monocular projection factors next to the stereo factors (include/vus_mono.h) for the tests:
sensor_ref.SensorBA whose observation list holds both kinds.  A stereo row is the CPU oracle's stereo factor at the
camera pose C = X o S, as in SensorBA; a mono row is gtsam's GenericProjectionFactor<Pose3, Point3, Cal3_S2> written here
in matrix form,

    q = Rc^T (p - tc),  (u, v) = (cx + (fx x + s y) / z, cy + fy y / z),  b = ((u, v) - m) / sigma_mono,
    D = d(u, v)/dq / sigma_mono,  H2 = D Rc^T,  H1_cam = D [ [q]x, -I ],

placed in rows 0 and 2 of the factor's three (row 1, the stereo factor's uR, is zero and adds to nothing).  Cheirality
(z <= 0): b = 2 fx / sigma_mono on both rows, zero Jacobians.  The robust weights (d^2 over the rows a factor has), the
linearisation, the step evaluation, the damped solve and the LM are inherited unchanged."""
import numpy as np

import sensor_ref

IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def mono_project(T, p, K):
    """(u, v) of point p from the camera pose T (flat12) with K = (fx, fy, s, cx, cy), and the depth z"""
    T, p = np.asarray(T, np.float64), np.asarray(p, np.float64)
    x, y, z = T[:9].reshape(3, 3).T @ (p - T[9:])
    return np.array([K[3] + (K[0] * x + K[2] * y) / z, K[4] + K[1] * y / z]), z


def mono_factor(T, p, m, K, w):
    """whitened r [2], H1 [2,6] (camera tangent [omega, v]), H2 [2,3] of one projection factor; m = (u, v), w = 1 / sigma"""
    T, p = np.asarray(T, np.float64), np.asarray(p, np.float64)
    R, t = T[:9].reshape(3, 3), T[9:]
    fx, fy, s = K[0], K[1], K[2]
    q = R.T @ (p - t)
    x, y, z = q
    if z <= 0.0:
        return np.full(2, 2.0 * fx * w), np.zeros((2, 6)), np.zeros((2, 3))
    uv, _ = mono_project(T, p, K)
    D = w * np.array([[fx / z, s / z, -(fx * x + s * y) / (z * z)], [0.0, fy / z, -fy * y / (z * z)]])
    return (uv - np.asarray(m, np.float64)[:2]) * w, D @ np.hstack([sensor_ref.skew(q), -np.eye(3)]), D @ R.T


class MonoBA(sensor_ref.SensorBA):
    """SensorBA with a flag per observation (L-order): nonzero = mono, `meas` row (u, ignored, v), calibration mono_K =
    (fx, fy, s, cx, cy) and sigma mono_sigma.  S = None: no extrinsic (the identity, which composes exactly)."""

    def __init__(self, O, pk, K, sigma, kind, k, S, is_mono, mono_K, mono_sigma, priors=None):
        super().__init__(O, pk, K, sigma, kind, k, IDENTITY if S is None else S, priors)
        self.is_mono = np.asarray(is_mono).reshape(-1) != 0
        assert len(self.is_mono) == self.nO
        self.mono_K = np.asarray(mono_K, np.float64).reshape(5)
        self.mono_w = 1.0 / float(mono_sigma)

    def factors(self, poses, points, jac=True):
        """whitened r [n,3], H1 [n,3,6] (body tangent), H2 [n,3,3], L-order; row 1 of a mono observation is zero"""
        cams = np.stack([sensor_ref.compose(p, self.S) for p in np.asarray(poses, np.float64).reshape(-1, 12)])
        r = np.zeros((self.nO, 3)); H1 = np.zeros((self.nO, 3, 6)); H2 = np.zeros((self.nO, 3, 3))
        for a in range(self.nO):
            T, p = cams[self.op[a]], points[self.ol[a]]
            if self.is_mono[a]:
                r[a, ::2], H1[a, ::2], H2[a, ::2] = mono_factor(T, p, self.meas[a, ::2], self.mono_K, self.mono_w)
            else:
                r[a], H1[a], H2[a] = self.O.stereo_factor(T, p, self.meas[a], self.K, self.w_sig)
        return r, H1 @ self.Ad, H2
