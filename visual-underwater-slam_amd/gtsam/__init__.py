"""A gtsam-shaped module: the drop-in boundary of the BA hot path.

`/root/reference/batch.py` builds its factor graph and solves it exclusively through the Python
`gtsam` API (import list batch.py:19-26; graph build :270-305; solve :337; read-back :57-68).  This
module exposes the same names with the same argument meaning, so that

    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import B, V, X, L

is the only change batch.py needs for the stereo path; `LevenbergMarquardtOptimizer.optimize()` then
runs on the MI355X kernels (ba.py / csrc/ba.hip).

Scope: GenericStereoFactor3D, GenericProjectionFactorCal3_S2, PriorFactorPose3, PriorFactorVector,
the partial absolute measurements on a pose GPSFactor, GPSFactorArm, PoseTranslationPrior3D and PoseRotationPrior3D
(position, position of a transponder off the body origin, attitude; include/vus_pose_meas.h), ImuFactor (with
PreintegratedImuMeasurements), CombinedImuFactor (with PreintegratedCombinedMeasurements; one bias per keyframe,
include/vus_combined_imu.h) and the DVL velocity factor (DvlVelocityFactor, the well-formed
replacement of the reference's CustomFactor) are solved on the GPU.  A generic gtsam.CustomFactor
(arbitrary Python callback) can be constructed and added, but optimize() refuses it, loudly.

Host-side classes here hold plain numpy values; no BA arithmetic happens in Python.
Errors surface as RuntimeError, as pybind11 does for gtsam's C++ exceptions.
"""
import math
from array import array
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import symbol_shorthand  # noqa: F401
from . import utils  # noqa: F401
from .symbol_shorthand import symbol, symbolChr, symbolIndex  # noqa: F401

__all__ = [
    "Point3", "Rot3", "Pose3", "Cal3_S2Stereo", "Cal3_S2", "StereoPoint2", "noiseModel", "imuBias",
    "GenericStereoFactor3D", "PriorFactorPose3", "PriorFactorVector", "PriorFactorPoint3",
    "PriorFactorConstantBias", "BetweenFactorConstantBias", "BetweenFactorPose3", "ImuFactor", "CombinedImuFactor", "PreintegrationCombinedParams",
    "PreintegratedCombinedMeasurements", "CustomFactor", "DvlVelocityFactor",
    "PreintegrationParams", "PreintegratedImuMeasurements", "NavState", "ISAM2", "ConstantTwistScenario",
    "PinholeCameraCal3_S2",
    "NonlinearFactorGraph", "Values", "LevenbergMarquardtParams", "LevenbergMarquardtOptimizer",
    "StereoFactorBlock", "symbol_shorthand", "symbol",
    "Point2", "GenericProjectionFactorCal3_S2", "ProjectionFactorBlock",
    "GPSFactor", "GPSFactorArm", "PoseTranslationPrior3D", "PoseRotationPrior3D",
]


# ---------------------------------------------------------------------------------------------
# geometry
def Point3(x=0.0, y=0.0, z=0.0):
    """gtsam.Point3 is a numpy 3-vector in the Python wrapper (batch.py:46,84,132,166)."""
    if isinstance(x, (list, tuple, np.ndarray)):
        return np.asarray(x, dtype=float).reshape(3).copy()
    return np.array([x, y, z], dtype=float)


def Point2(x=0.0, y=0.0):
    """gtsam.Point2 is a numpy 2-vector in the Python wrapper."""
    if isinstance(x, (list, tuple, np.ndarray)):
        return np.asarray(x, dtype=float).reshape(2).copy()
    return np.array([x, y], dtype=float)


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


class Rot3:
    def __init__(self, R=None):
        self._R = np.eye(3) if R is None else np.asarray(R, dtype=float).reshape(3, 3).copy()

    @staticmethod
    def Quaternion(w, x, y, z):                    # batch.py:47,131  (w first)
        n = math.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        return Rot3([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    @staticmethod
    def Rodrigues(wx, wy=None, wz=None):           # batch.py:190
        w = np.asarray(wx, dtype=float).reshape(3) if wy is None else np.array([wx, wy, wz], dtype=float)
        return Rot3.Expmap(w)

    @staticmethod
    def Expmap(w):
        w = np.asarray(w, dtype=float).reshape(3)
        th2 = float(w @ w)
        K = _skew(w)
        if th2 <= np.finfo(float).eps:
            return Rot3(np.eye(3) + K)
        th = math.sqrt(th2)
        return Rot3(np.eye(3) + math.sin(th) / th * K + 2.0 * math.sin(0.5 * th) ** 2 / th2 * (K @ K))

    @staticmethod
    def Rx(t):
        c, s = math.cos(t), math.sin(t)
        return Rot3([[1, 0, 0], [0, c, -s], [0, s, c]])

    @staticmethod
    def Ry(t):
        c, s = math.cos(t), math.sin(t)
        return Rot3([[c, 0, s], [0, 1, 0], [-s, 0, c]])

    @staticmethod
    def Rz(t):
        c, s = math.cos(t), math.sin(t)
        return Rot3([[c, -s, 0], [s, c, 0], [0, 0, 1]])

    @staticmethod
    def Ypr(y, p, r):
        return Rot3(Rot3.Rz(y)._R @ Rot3.Ry(p)._R @ Rot3.Rx(r)._R)

    def matrix(self):
        return self._R.copy()

    def inverse(self):
        return Rot3(self._R.T)

    def compose(self, other):
        return Rot3(self._R @ other._R)

    def rotate(self, p):
        return self._R @ np.asarray(p, dtype=float).reshape(3)

    def __mul__(self, other):
        return self.compose(other)

    def equals(self, other, tol=1e-9):
        return bool(np.allclose(self._R, other._R, atol=tol))

    def __repr__(self):
        return f"Rot3(\n{self._R}\n)"


class Pose3:
    """Camera/body pose: rotation R and translation t (body-to-world), gtsam.Pose3."""

    def __init__(self, r=None, t=None):
        if r is None:
            self._R, self._t = np.eye(3), np.zeros(3)
        elif isinstance(r, Pose3):
            self._R, self._t = r._R.copy(), r._t.copy()
        elif isinstance(r, Rot3):
            self._R = r.matrix()
            self._t = np.zeros(3) if t is None else np.asarray(t, dtype=float).reshape(3).copy()
        else:
            M = np.asarray(r, dtype=float)
            if M.shape != (4, 4):
                raise RuntimeError("Pose3(): expected (Rot3, Point3), a 4x4 matrix, or nothing")
            self._R, self._t = M[:3, :3].copy(), M[:3, 3].copy()

    # accessors used by batch.py:62,134-135,213
    def x(self):
        return float(self._t[0])

    def y(self):
        return float(self._t[1])

    def z(self):
        return float(self._t[2])

    def rotation(self):
        return Rot3(self._R)

    def translation(self):
        return self._t.copy()

    def matrix(self):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = self._R, self._t
        return M

    def inverse(self):
        return Pose3(Rot3(self._R.T), -self._R.T @ self._t)

    def compose(self, other):
        return Pose3(Rot3(self._R @ other._R), self._t + self._R @ other._t)

    def __mul__(self, other):
        return self.compose(other)

    def between(self, other):
        return self.inverse().compose(other)

    def transformFrom(self, p):
        return self._R @ np.asarray(p, dtype=float).reshape(3) + self._t

    def transformTo(self, p):
        return self._R.T @ (np.asarray(p, dtype=float).reshape(3) - self._t)

    def equals(self, other, tol=1e-9):
        return bool(np.allclose(self._R, other._R, atol=tol) and np.allclose(self._t, other._t, atol=tol))

    # tangent space: (omega, v), retract T Exp(xi), local Log(T^-1 T2) -- the conventions of the GPU kernels
    @staticmethod
    def Expmap(xi):
        xi = np.asarray(xi, dtype=float).reshape(6)
        w, v = xi[:3], xi[3:]
        R = Rot3.Expmap(w)._R
        th2 = float(w @ w)
        b, c = 0.5, 1.0 / 6.0                     # t = V v = v + b w x v + c w x (w x v), as csrc/se3_device.h sums it
        if th2 > np.finfo(float).eps:
            th = math.sqrt(th2)
            b, c = 2.0 * math.sin(0.5 * th) ** 2 / th2, (th - math.sin(th)) / (th2 * th)
        wv = np.cross(w, v)
        t = v + b * wv + c * np.cross(w, wv)
        return Pose3(Rot3(R), t)

    @staticmethod
    def Logmap(T):
        R, t = T._R, T._t
        tr = float(np.trace(R))
        if tr < -0.4:                             # above 134 degrees: atan2 and the symmetric part (csrc/se3_device.h)
            v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
            c = 0.5 * (tr - 1.0)
            th = math.atan2(0.5 * float(np.linalg.norm(v)), c)
            i = int(np.argmax(np.diag(R)))
            a = 0.5 * (R[:, i] + R[i, :])
            a[i] -= c
            w = th / float(np.linalg.norm(a)) * a
            if float(v @ a) < 0.0:
                w = -w
        else:
            tr3 = tr - 3.0
            if tr3 < -1e-7:
                th = math.acos((tr - 1.0) / 2.0)
                mag = th / (2.0 * math.sin(th))
            else:
                mag = 0.5 - tr3 / 12.0
            w = mag * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        th = float(np.linalg.norm(w))
        if th < 1e-10:
            return np.concatenate([w, t - 0.5 * np.cross(w, t)])
        k = w / th
        WT = np.cross(k, t)
        v = t - (0.5 * th) * WT + (1.0 - th / (2.0 * math.tan(0.5 * th))) * np.cross(k, WT)
        return np.concatenate([w, v])

    def localCoordinates(self, other):
        return Pose3.Logmap(self.between(other))

    def retract(self, xi):
        return self.compose(Pose3.Expmap(xi))

    def flat12(self):
        """Row-major R followed by t: the device layout of include/vus.h."""
        return np.concatenate([self._R.reshape(-1), self._t])

    @staticmethod
    def from_flat12(v):
        v = np.asarray(v, dtype=float).reshape(12)
        return Pose3(Rot3(v[:9].reshape(3, 3)), v[9:])

    def __repr__(self):
        return f"Pose3(R=\n{self._R},\n t={self._t})"


class Cal3_S2Stereo:
    def __init__(self, fx=1.0, fy=1.0, s=0.0, u0=0.0, v0=0.0, b=1.0):   # batch.py:115
        self._v = (float(fx), float(fy), float(s), float(u0), float(v0), float(b))

    def fx(self):
        return self._v[0]

    def fy(self):
        return self._v[1]

    def skew(self):
        return self._v[2]

    def px(self):
        return self._v[3]

    def py(self):
        return self._v[4]

    def baseline(self):
        return self._v[5]

    def vector6(self):
        return np.array(self._v)

    def equals(self, other, tol=1e-9):
        return bool(np.allclose(self._v, other._v, atol=tol))


class Cal3_S2:
    """gtsam.Cal3_S2(fx, fy, s, u0, v0): the five-parameter pinhole calibration.  Its skew IS used by the projection."""

    def __init__(self, fx=1.0, fy=1.0, s=0.0, u0=0.0, v0=0.0):
        self._v = (float(fx), float(fy), float(s), float(u0), float(v0))

    def fx(self):
        return self._v[0]

    def fy(self):
        return self._v[1]

    def skew(self):
        return self._v[2]

    def px(self):
        return self._v[3]

    def py(self):
        return self._v[4]

    def vector(self):
        """(fx, fy, s, u0, v0)"""
        return np.array(self._v)

    def K(self):
        fx, fy, s, u0, v0 = self._v
        return np.array([[fx, s, u0], [0.0, fy, v0], [0.0, 0.0, 1.0]])

    def equals(self, other, tol=1e-9):
        return bool(np.allclose(self._v, other._v, atol=tol))

    def __repr__(self):
        return "Cal3_S2(fx={}, fy={}, s={}, u0={}, v0={})".format(*self._v)


class StereoPoint2:
    def __init__(self, uL=0.0, uR=0.0, v=0.0):                           # batch.py:301
        self._m = np.array([uL, uR, v], dtype=float)

    def uL(self):
        return float(self._m[0])

    def uR(self):
        return float(self._m[1])

    def v(self):
        return float(self._m[2])

    def vector(self):
        return self._m.copy()


# ---------------------------------------------------------------------------------------------
# noise models (batch.py:95-98,118,189)
class _NoiseModel:
    def __init__(self, sigmas):
        self._sigmas = np.asarray(sigmas, dtype=float).reshape(-1).copy()
        if (self._sigmas <= 0).any():
            raise RuntimeError("noise model sigmas must be positive")

    def sigmas(self):
        return self._sigmas.copy()

    def dim(self):
        return int(self._sigmas.size)

    def is_isotropic(self):
        return bool(np.all(self._sigmas == self._sigmas[0]))


class _Diagonal(_NoiseModel):
    @staticmethod
    def Sigmas(sigmas):
        return _Diagonal(sigmas)

    @staticmethod
    def Variances(v):
        return _Diagonal(np.sqrt(np.asarray(v, dtype=float)))

    @staticmethod
    def Precisions(p):
        return _Diagonal(1.0 / np.sqrt(np.asarray(p, dtype=float)))


class _Isotropic(_NoiseModel):
    @staticmethod
    def Sigma(dim, sigma):
        return _Isotropic(np.full(int(dim), float(sigma)))

    @staticmethod
    def Variance(dim, variance):
        return _Isotropic(np.full(int(dim), math.sqrt(float(variance))))


class _Unit(_NoiseModel):
    @staticmethod
    def Create(dim):
        return _Unit(np.ones(int(dim)))


class _Gaussian(_NoiseModel):
    """gtsam.noiseModel.Gaussian: a full-covariance model, held as the upper-triangular R with R^T R = cov^-1; a vector is
    whitened as R v, a Jacobian as R H.  R() is the upper Cholesky factor of the information matrix (positive diagonal)
    whichever constructor was used -- GTSAM's behaviour as recalled, not checked against a build (SqrtInformation there
    keeps the matrix it is given); any R with R^T R = cov^-1 gives the same error.  Covariance / Information /
    SqrtInformation return the Diagonal model for an exactly diagonal matrix (GTSAM's smart = true).
    BetweenFactorPose3 takes it (include/vus_between.h, sqrt_info); every other factor refuses it at construction."""

    def __init__(self, R):
        self._R = R
        self._cov = np.linalg.inv(R.T @ R)
        self._cov = 0.5 * (self._cov + self._cov.T)
        super().__init__(np.sqrt(np.diag(self._cov)))

    @staticmethod
    def _square(M, what):
        M = np.array(M, dtype=float)
        if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] == 0:
            raise RuntimeError(f"noiseModel.Gaussian.{what}: a square matrix is expected, not an array of shape {M.shape}")
        if not np.isfinite(M).all():
            raise RuntimeError(f"noiseModel.Gaussian.{what}: the matrix must be finite")
        return M

    @staticmethod
    def _from_spd(M, what, inverse):
        """The model of the symmetric positive definite M = the information (or, with `inverse`, the covariance)."""
        M = _Gaussian._square(M, what)
        if np.abs(M - M.T).max() > 1e-9 * np.abs(M).max():
            raise RuntimeError(f"noiseModel.Gaussian.{what}: the matrix is not symmetric (relative 1e-9)")
        M = 0.5 * (M + M.T)
        try:
            np.linalg.cholesky(M)
            info = np.linalg.inv(M) if inverse else M
            R = np.linalg.cholesky(0.5 * (info + info.T)).T
        except np.linalg.LinAlgError:
            raise RuntimeError(f"noiseModel.Gaussian.{what}: the matrix is not positive definite") from None
        if not np.isfinite(R).all():
            raise RuntimeError(f"noiseModel.Gaussian.{what}: the matrix is not positive definite")
        if not (M - np.diag(np.diag(M))).any():
            return _Diagonal(np.sqrt(np.diag(M)) if inverse else 1.0 / np.sqrt(np.diag(M)))
        return _Gaussian(np.triu(R))

    @staticmethod
    def Covariance(covariance, smart=True):
        return _Gaussian._from_spd(covariance, "Covariance", True)

    @staticmethod
    def Information(information, smart=True):
        return _Gaussian._from_spd(information, "Information", False)

    @staticmethod
    def SqrtInformation(R, smart=True):
        R = _Gaussian._square(R, "SqrtInformation")
        if np.linalg.matrix_rank(R) < R.shape[0]:
            raise RuntimeError("noiseModel.Gaussian.SqrtInformation: the matrix is singular")
        return _Gaussian._from_spd(R.T @ R, "SqrtInformation", False)

    def R(self):
        return self._R.copy()

    def information(self):
        return self._R.T @ self._R

    def covariance(self):
        return self._cov.copy()

    def whiten(self, v):
        return self._R @ np.asarray(v, dtype=float).reshape(-1)

    def Whiten(self, H):
        return self._R @ np.asarray(H, dtype=float)

    def is_isotropic(self):
        return False


def _sqrt_info_of(model):
    """The [d, d] whitening matrix of a Gaussian or diagonal model (the noise of a Robust one): R, or diag(1 / sigma)."""
    noise = model._noise if isinstance(model, _Robust) else model
    return noise._R.copy() if isinstance(noise, _Gaussian) else np.diag(1.0 / noise._sigmas)


def _is_full(model):
    """The model (or the noise of a Robust one) is a full-covariance noiseModel.Gaussian."""
    return isinstance(model._noise if isinstance(model, _Robust) else model, _Gaussian)


def _refuse_full(model, what):
    if isinstance(model, _NoiseModel) and _is_full(model):
        raise NotImplementedError(f"{what}: a full-covariance noiseModel.Gaussian is supported on BetweenFactorPose3 only; use a "
                                  "Diagonal / Isotropic / Unit model here")


class _MEstimator:
    """gtsam.noiseModel.mEstimator.Base: a robust loss rho(d) of the whitened residual norm d and its IRLS weight
    w(d) = rho'(d) / d, GTSAM's default Block reweighting (one weight per factor).  `kind` is the VUS_LOSS_* number of
    include/vus_robust.h, `k` the parameter in whitened units."""
    kind = 0
    _name = "Gaussian"

    def __init__(self, k, reweight=None):
        k = float(k)
        if not (math.isfinite(k) and k > 0.0):
            raise RuntimeError(f"mEstimator.{self._name}: parameter {k} must be finite and > 0")
        if reweight not in (None, 1, "Block"):
            raise NotImplementedError("only the Block reweight scheme (gtsam's default) is supported")
        self.k = k

    @classmethod
    def Create(cls, k, reweight=None):
        return cls(k, reweight)

    def modelParameter(self):
        return self.k

    def weight(self, d):
        return float(self._wl(abs(float(d)))[0])

    def sqrtWeight(self, d):
        return math.sqrt(self.weight(d))

    def loss(self, d):
        return float(self._wl(abs(float(d)))[1])

    def _wl(self, d):
        raise NotImplementedError

    def equals(self, other, tol=1e-9):
        return type(other) is type(self) and abs(other.k - self.k) <= tol

    def __repr__(self):
        return f"mEstimator.{self._name}({self.k:g})"


class _Huber(_MEstimator):
    kind, _name = 1, "Huber"

    def _wl(self, d):
        k = self.k
        return (1.0, 0.5 * d * d) if d <= k else (k / d, k * d - 0.5 * k * k)


class _Cauchy(_MEstimator):
    kind, _name = 2, "Cauchy"

    def _wl(self, d):
        k2 = self.k * self.k
        return k2 / (k2 + d * d), 0.5 * k2 * math.log1p(d * d / k2)


class _Tukey(_MEstimator):
    kind, _name = 3, "Tukey"

    def _wl(self, d):
        c2 = self.k * self.k
        if d > self.k:
            return 0.0, c2 / 6.0
        t = 1.0 - d * d / c2
        return t * t, c2 / 6.0 * (1.0 - t * t * t)


class _GemanMcClure(_MEstimator):
    kind, _name = 4, "GemanMcClure"

    def _wl(self, d):
        c2, d2 = self.k * self.k, d * d
        return c2 * c2 / ((c2 + d2) * (c2 + d2)), 0.5 * c2 * d2 / (c2 + d2)


class _Welsch(_MEstimator):
    kind, _name = 5, "Welsch"

    def _wl(self, d):
        x = d * d / (self.k * self.k)
        return math.exp(-x), -0.5 * self.k * self.k * math.expm1(-x)


class _mEstimator:  # namespace (gtsam.noiseModel.mEstimator)
    Base = _MEstimator
    Huber = _Huber
    Cauchy = _Cauchy
    Tukey = _Tukey
    GemanMcClure = _GemanMcClure
    Welsch = _Welsch


class _Robust(_NoiseModel):
    """gtsam.noiseModel.Robust.Create(mEstimator, noise): the whitening of `noise` followed by IRLS reweighting with the
    mEstimator (Block scheme).  The GPU optimizer supports it on stereo factors over an isotropic noise model."""

    def __init__(self, robust: _MEstimator, noise: _NoiseModel):
        if not isinstance(robust, _MEstimator):
            raise RuntimeError("Robust.Create: the first argument must be a noiseModel.mEstimator")
        if not isinstance(noise, _NoiseModel) or isinstance(noise, _Robust):
            raise RuntimeError("Robust.Create: the second argument must be a Gaussian noise model")
        super().__init__(noise.sigmas())
        self._robust, self._noise = robust, noise

    @staticmethod
    def Create(robust, noise):
        return _Robust(robust, noise)

    def robust(self):
        return self._robust

    def noise(self):
        return self._noise

    def is_isotropic(self):
        return self._noise.is_isotropic()


def _refuse_robust(model, what):
    if isinstance(model, _Robust):
        raise NotImplementedError(f"{what}: a noiseModel.Robust model is supported on stereo factors only "
                                  "(GenericStereoFactor3D, StereoFactorBlock); use a Gaussian noise model here")


def _stereo_model_key(model):
    """What makes two stereo noise models the same model: sigmas, robust kind and parameter."""
    rob = model._robust if isinstance(model, _Robust) else None
    return (tuple(model._sigmas.tolist()), rob.kind if rob else 0, rob.k if rob else 0.0)


class noiseModel:  # namespace, as in gtsam
    Base = _NoiseModel
    Diagonal = _Diagonal
    Gaussian = _Gaussian
    Isotropic = _Isotropic
    Unit = _Unit
    Robust = _Robust
    mEstimator = _mEstimator


class _ConstantBias:
    def __init__(self, biasAcc=None, biasGyro=None):
        self._a = np.zeros(3) if biasAcc is None else np.asarray(biasAcc, dtype=float).reshape(3)
        self._g = np.zeros(3) if biasGyro is None else np.asarray(biasGyro, dtype=float).reshape(3)

    def vector(self):
        return np.concatenate([self._a, self._g])

    def accelerometer(self):
        return self._a.copy()

    def gyroscope(self):
        return self._g.copy()


class imuBias:  # namespace (batch.py:92)
    ConstantBias = _ConstantBias


# ---------------------------------------------------------------------------------------------
# factors
class _Factor:
    def __init__(self, keys):
        self._keys = [int(k) for k in keys]

    def keys(self):
        return list(self._keys)

    def size(self):
        return len(self._keys)


def _sensor_pose(body_P_sensor):
    """The stored form of a factor's body_P_sensor argument: None or an own Pose3."""
    if body_P_sensor is None:
        return None
    if not isinstance(body_P_sensor, Pose3):
        raise RuntimeError("body_P_sensor must be a Pose3 or None")
    return Pose3(body_P_sensor)


def _same_sensor(a, b):
    """Two stored extrinsics agree: both None, or equal poses in gtsam's sense of Pose3::equals(tol = 1e-12), every
    entry within the ABSOLUTE tolerance (Pose3.equals above also grants numpy's relative 1e-5)."""
    if a is None or b is None:
        return a is None and b is None
    return a is b or bool(np.abs(a.flat12() - b.flat12()).max() <= 1e-12)


class GenericStereoFactor3D(_Factor):
    """GenericStereoFactor<Pose3, Point3>(measured, model, poseKey, landmarkKey, K, body_P_sensor=None)
    (batch.py:300-304).  With a body_P_sensor the pose variable is the vehicle body and the left camera sits at
    pose o body_P_sensor; one graph holds one extrinsic (or none)."""

    def __init__(self, measured: StereoPoint2, model: _NoiseModel, poseKey: int, landmarkKey: int,
                 K: Cal3_S2Stereo, body_P_sensor: Optional[Pose3] = None):
        super().__init__([poseKey, landmarkKey])
        _refuse_full(model, "GenericStereoFactor3D")
        if model.dim() != 3:
            raise RuntimeError("GenericStereoFactor3D needs a 3-dimensional noise model")
        self._measured, self._model, self._K = measured, model, K
        self._sensor = _sensor_pose(body_P_sensor)

    def body_P_sensor(self):
        """A copy of the camera-to-body extrinsic, or None."""
        return None if self._sensor is None else Pose3(self._sensor)

    def measured(self):
        return self._measured

    def calibration(self):
        return self._K

    def noiseModel(self):
        return self._model


class GenericProjectionFactorCal3_S2(_Factor):
    """GenericProjectionFactor<Pose3, Point3, Cal3_S2>(measured, model, poseKey, pointKey, K, body_P_sensor=None): a
    landmark seen in one image, residual project(pose o body_P_sensor, point) - measured under a 2-dimensional model.
    It shares the graph with GenericStereoFactor3D factors (include/vus_mono.h): one Cal3_S2, one isotropic model and one
    extrinsic for all mono factors of a graph; the extrinsic and, for robust models, the mEstimator are those of the
    stereo factors too (the sigmas may differ).
    There is no observability check: a landmark held by a single monocular sighting has a rank-2 information block and is
    kept finite by the Levenberg-Marquardt damping alone -- as in GTSAM, until its linear solver throws.  A
    PriorFactorPoint3 on such a landmark makes it determinate (and, with a PriorFactorPose3, fixes the scale of a graph of
    monocular factors only)."""

    def __init__(self, measured, model: _NoiseModel, poseKey: int, pointKey: int, K: Cal3_S2,
                 body_P_sensor: Optional[Pose3] = None):
        super().__init__([poseKey, pointKey])
        _refuse_full(model, "GenericProjectionFactorCal3_S2")
        if model.dim() != 2:
            raise RuntimeError("GenericProjectionFactorCal3_S2 needs a 2-dimensional noise model")
        if not isinstance(K, Cal3_S2):
            raise RuntimeError("GenericProjectionFactorCal3_S2 needs a Cal3_S2 calibration")
        self._measured = Point2(np.asarray(measured, dtype=float).reshape(2))
        self._model, self._K = model, K
        self._sensor = _sensor_pose(body_P_sensor)

    def body_P_sensor(self):
        """A copy of the camera-to-body extrinsic, or None."""
        return None if self._sensor is None else Pose3(self._sensor)

    def measured(self):
        return self._measured.copy()

    def calibration(self):
        return self._K

    def noiseModel(self):
        return self._model


class ProjectionFactorBlock(_Factor):
    """EXTENSION (not in gtsam): many GenericProjectionFactorCal3_S2 factors sharing one noise model, one calibration
    and one extrinsic, held as arrays -- what StereoFactorBlock is to GenericStereoFactor3D.  measured: [n, 2] (u, v)."""

    def __init__(self, measured, model: _NoiseModel, poseKeys, pointKeys, K: Cal3_S2,
                 body_P_sensor: Optional[Pose3] = None):
        self.meas = np.ascontiguousarray(measured, dtype=float).reshape(-1, 2)
        self.pose_keys = np.ascontiguousarray(poseKeys, dtype=np.int64).reshape(-1)
        self.landmark_keys = np.ascontiguousarray(pointKeys, dtype=np.int64).reshape(-1)
        if not (len(self.meas) == len(self.pose_keys) == len(self.landmark_keys)):
            raise RuntimeError("ProjectionFactorBlock: arrays differ in length")
        _refuse_full(model, "ProjectionFactorBlock")
        if model.dim() != 2:
            raise RuntimeError("ProjectionFactorBlock needs a 2-dimensional noise model")
        if not isinstance(K, Cal3_S2):
            raise RuntimeError("ProjectionFactorBlock needs a Cal3_S2 calibration")
        self._model, self._K = model, K
        self._sensor = _sensor_pose(body_P_sensor)
        self._keys = None

    def body_P_sensor(self):
        """A copy of the camera-to-body extrinsic of every factor of the block, or None."""
        return None if self._sensor is None else Pose3(self._sensor)

    def calibration(self):
        return self._K

    def noiseModel(self):
        return self._model

    def keys(self):
        return np.unique(np.concatenate([self.pose_keys, self.landmark_keys])).tolist()

    def size(self):
        return len(self.meas)

    def __len__(self):
        return len(self.meas)


class StereoFactorBlock(_Factor):
    """EXTENSION (not in gtsam): many GenericStereoFactor3D factors sharing one noise model and one
    calibration, held as arrays.  It is the vectorised form of the emission loop batch.py:296-305 for
    graphs with millions of observations, where one Python object per factor is the bottleneck."""

    def __init__(self, measured, model: _NoiseModel, poseKeys, landmarkKeys, K: Cal3_S2Stereo,
                 body_P_sensor: Optional[Pose3] = None):
        self.meas = np.ascontiguousarray(measured, dtype=float).reshape(-1, 3)
        self.pose_keys = np.ascontiguousarray(poseKeys, dtype=np.int64).reshape(-1)
        self.landmark_keys = np.ascontiguousarray(landmarkKeys, dtype=np.int64).reshape(-1)
        if not (len(self.meas) == len(self.pose_keys) == len(self.landmark_keys)):
            raise RuntimeError("StereoFactorBlock: arrays differ in length")
        _refuse_full(model, "StereoFactorBlock")
        if model.dim() != 3:
            raise RuntimeError("StereoFactorBlock needs a 3-dimensional noise model")
        self._model, self._K = model, K
        self._sensor = _sensor_pose(body_P_sensor)
        self._keys = None

    def body_P_sensor(self):
        """A copy of the camera-to-body extrinsic of every factor of the block, or None."""
        return None if self._sensor is None else Pose3(self._sensor)

    def keys(self):
        return np.unique(np.concatenate([self.pose_keys, self.landmark_keys])).tolist()

    def size(self):
        return len(self.meas)

    def __len__(self):
        return len(self.meas)


class _PriorFactor(_Factor):
    def __init__(self, key, prior, model):
        super().__init__([key])
        self._prior, self._model = prior, model

    def prior(self):
        return self._prior

    def noiseModel(self):
        return self._model


class PriorFactorPose3(_PriorFactor):
    def __init__(self, key, prior: Pose3, model: _NoiseModel):           # batch.py:281
        _refuse_full(model, "PriorFactorPose3")
        if model.dim() != 6:
            raise RuntimeError("PriorFactorPose3 needs a 6-dimensional noise model")
        _refuse_robust(model, "PriorFactorPose3")
        super().__init__(key, Pose3(prior), model)


class PriorFactorVector(_PriorFactor):
    def __init__(self, key, prior, model: _NoiseModel):                  # batch.py:282
        prior = np.asarray(prior, dtype=float).reshape(-1).copy()
        _refuse_full(model, type(self).__name__)
        if model.dim() != prior.size:
            raise RuntimeError("PriorFactorVector: noise model dimension differs from the vector's")
        _refuse_robust(model, "PriorFactorVector")
        super().__init__(key, prior, model)


class PriorFactorPoint3(PriorFactorVector):
    """gtsam.PriorFactorPoint3(key, prior, model): error 0.5 |(p - prior) / sigma|^2 under a 3-dimensional Diagonal /
    Isotropic / Unit model.  On a landmark that stereo or monocular factors observe it is solved on the GPU with them
    (include/vus_point_prior.h; several priors on one landmark are summed); on a landmark nothing observes it decouples
    and stays on the host."""

    def __init__(self, key, prior, model: _NoiseModel):
        if np.asarray(prior, dtype=float).size != 3:
            raise RuntimeError("PriorFactorPoint3 needs a 3-vector prior")
        if model.dim() != 3:
            raise RuntimeError("PriorFactorPoint3 needs a 3-dimensional noise model")
        super().__init__(key, prior, model)


class PriorFactorConstantBias(_PriorFactor):
    def __init__(self, key, prior: _ConstantBias, model: _NoiseModel):
        _refuse_full(model, "PriorFactorConstantBias")
        super().__init__(key, prior, model)


class BetweenFactorConstantBias(_Factor):
    def __init__(self, key1, key2, measured, model):
        super().__init__([key1, key2])
        _refuse_full(model, "BetweenFactorConstantBias")
        self._measured, self._model = measured, model


class BetweenFactorPose3(_Factor):
    """gtsam.BetweenFactorPose3(key1, key2, measured, model): error 0.5 |Log(measured^-1 (X1^-1 X2))|^2 in the whitening of
    a 6-dimensional Diagonal / Isotropic / Unit model or a full-covariance noiseModel.Gaussian (whitening R r, R^T R =
    cov^-1), optionally wrapped in noiseModel.Robust (include/vus_between.h).
    Odometry (consecutive keys) and loop closures (any two keyframes) alike; the two keys must differ."""

    def __init__(self, key1, key2, measured: Pose3, model: _NoiseModel):
        super().__init__([key1, key2])
        if model.dim() != 6:
            raise RuntimeError("BetweenFactorPose3 needs a 6-dimensional noise model")
        if self._keys[0] == self._keys[1]:
            raise ValueError(f"BetweenFactorPose3: both keys are {symbol_shorthand.key_string(self._keys[0])}")
        if not isinstance(measured, Pose3):
            raise RuntimeError("BetweenFactorPose3: the measurement must be a Pose3")
        self._measured, self._model = Pose3(measured), model

    def measured(self):
        return Pose3(self._measured)

    def noiseModel(self):
        return self._model


class _PoseMeasFactor(_Factor):
    """A partial absolute measurement on one Pose3 (include/vus_pose_meas.h): three residual rows under a 3-dimensional
    Diagonal / Isotropic / Unit model, optionally wrapped in noiseModel.Robust.  `_kind` is the VUS_POSE_MEAS_* number and
    `_row9()` the factor's nine measurement doubles."""
    _kind = 0

    def __init__(self, key, model):
        super().__init__([key])
        what = type(self).__name__
        if not isinstance(model, _NoiseModel):
            raise RuntimeError(f"{what}: the last argument must be a noise model")
        _refuse_full(model, what)
        if model.dim() != 3:
            raise RuntimeError(f"{what} needs a 3-dimensional noise model, not one of dimension {model.dim()}")
        self._model = model

    def noiseModel(self):
        return self._model

    @staticmethod
    def _point(p, what):
        a = np.asarray(p, dtype=float)
        if a.size != 3 or not np.isfinite(a).all():
            raise RuntimeError(f"{what} must be a finite 3-vector")
        return a.reshape(3).copy()


class GPSFactor(_PoseMeasFactor):
    """gtsam.GPSFactor(key, gpsIn, model): the position of the pose measured in the world (navigation) frame, error
    0.5 |(t - gpsIn) / sigma|^2.  A depth fix is this factor with Diagonal.Sigmas([big, big, sigma_z])."""

    def __init__(self, key, gpsIn, model: _NoiseModel):
        super().__init__(key, model)
        self._m = self._point(gpsIn, "GPSFactor: gpsIn")

    def measurementIn(self):
        return self._m.copy()

    def _row9(self):
        return np.concatenate([self._m, np.zeros(6)])


class GPSFactorArm(_PoseMeasFactor):
    """gtsam.GPSFactorArm(key, gpsIn, leverArm, model): the world position of an antenna or transponder mounted at
    `leverArm` in the body frame, error 0.5 |(t + R leverArm - gpsIn) / sigma|^2."""

    def __init__(self, key, gpsIn, leverArm, model: _NoiseModel):
        super().__init__(key, model)
        self._m = self._point(gpsIn, "GPSFactorArm: gpsIn")
        self._arm = self._point(leverArm, "GPSFactorArm: leverArm")

    def measurementIn(self):
        return self._m.copy()

    def leverArm(self):
        return self._arm.copy()

    def _row9(self):
        return np.concatenate([self._m, self._arm, np.zeros(3)])


class PoseTranslationPrior3D(_PoseMeasFactor):
    """gtsam.PoseTranslationPrior3D(key, Point3 or Pose3, model): a prior on the translation of the pose in the world
    frame (of a Pose3 only the translation is used), error 0.5 |(t - measured) / sigma|^2."""

    def __init__(self, key, measured, model: _NoiseModel):
        super().__init__(key, model)
        self._m = self._point(measured.translation() if isinstance(measured, Pose3) else measured,
                              "PoseTranslationPrior3D: the measurement")

    def measured(self):
        return self._m.copy()

    def _row9(self):
        return np.concatenate([self._m, np.zeros(6)])


class PoseRotationPrior3D(_PoseMeasFactor):
    """gtsam.PoseRotationPrior3D(key, Rot3 or Pose3, model): a prior on the rotation of the pose (of a Pose3 only the
    rotation is used), error 0.5 |Log(measured^T R) / sigma|^2 with the identity as the Jacobian, as gtsam has it."""
    _kind = 1

    def __init__(self, key, measured, model: _NoiseModel):
        super().__init__(key, model)
        if isinstance(measured, Pose3):
            measured = measured.rotation()
        if not isinstance(measured, Rot3):
            raise RuntimeError("PoseRotationPrior3D: the measurement must be a Rot3 or a Pose3")
        R = measured.matrix()
        if not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-9 or np.linalg.det(R) <= 0.0:
            raise RuntimeError("PoseRotationPrior3D: the measured rotation is not a rotation matrix (orthonormal within 1e-9, "
                               "det > 0)")
        self._R = Rot3(R)

    def measured(self):
        return Rot3(self._R._R)

    def _row9(self):
        return self._R._R.reshape(9).copy()


class PreintegrationParams:
    """Holds the IMU noise parameters batch.py sets at :181-187 (consumed by gtsam/imu.py's Preintegrator when a PreintegratedImuMeasurements is built from them)."""

    def __init__(self, n_gravity):
        self.n_gravity = np.asarray(n_gravity, dtype=float)
        self.accelerometerCovariance = np.eye(3)
        self.gyroscopeCovariance = np.eye(3)
        self.integrationCovariance = np.eye(3)
        self.use2ndOrderCoriolis = False
        self.omegaCoriolis = np.zeros(3)

    @staticmethod
    def MakeSharedU(g=9.81):
        return PreintegrationParams([0.0, 0.0, -float(g)])

    @staticmethod
    def MakeSharedD(g=9.81):
        return PreintegrationParams([0.0, 0.0, float(g)])

    def setAccelerometerCovariance(self, c):
        self.accelerometerCovariance = np.asarray(c, dtype=float)

    def setGyroscopeCovariance(self, c):
        self.gyroscopeCovariance = np.asarray(c, dtype=float)

    def setIntegrationCovariance(self, c):
        self.integrationCovariance = np.asarray(c, dtype=float)

    def setUse2ndOrderCoriolis(self, f):
        self.use2ndOrderCoriolis = bool(f)

    def setOmegaCoriolis(self, w):
        self.omegaCoriolis = np.asarray(w, dtype=float)


class PreintegratedImuMeasurements:
    """gtsam.PreintegratedImuMeasurements(params, bias): on-manifold preintegration of the raw samples
    (batch.py:91,290,293), done on the host at graph-build time exactly like GTSAM does (imu.py)."""

    def __init__(self, params: PreintegrationParams, bias: Optional[_ConstantBias] = None):
        from .imu import Preintegrator
        self.params, self.bias = params, bias or _ConstantBias()
        self._pre = Preintegrator(self.bias.vector(), params.accelerometerCovariance, params.gyroscopeCovariance,
                                  params.integrationCovariance)

    def integrateMeasurement(self, acc, gyro, dt):
        self._pre.integrate(acc, gyro, dt)

    def resetIntegration(self):
        self._pre.reset()

    def deltaTij(self):
        return float(self._pre.dt)

    def deltaRij(self):
        return Rot3(self._pre.dR)

    def deltaPij(self):
        return self._pre.dP.copy()

    def deltaVij(self):
        return self._pre.dV.copy()

    def preintMeasCov(self):
        return self._pre.cov.copy()


class ImuFactor(_Factor):
    """ImuFactor(pose_i, vel_i, pose_j, vel_j, bias, pim)  (batch.py:238).  Like gtsam, the factor copies the
    preintegrated measurement at construction, so resetIntegration() right after (batch.py:293) is safe."""

    def __init__(self, pose_i, vel_i, pose_j, vel_j, bias, pim: PreintegratedImuMeasurements):
        super().__init__([pose_i, vel_i, pose_j, vel_j, bias])
        if pim._pre.dt <= 0.0:
            raise RuntimeError("ImuFactor: the preintegrated interval is empty (no IMU sample between the keyframes)")
        if pim.params.use2ndOrderCoriolis or np.any(pim.params.omegaCoriolis != 0):
            raise NotImplementedError("Coriolis terms are not implemented (batch.py:186-187 disables them)")
        self.pim = pim._pre.packed()
        self.W = pim._pre.whitening().reshape(-1)
        self.gravity = np.asarray(pim.params.n_gravity, dtype=float).copy()


class PreintegrationCombinedParams(PreintegrationParams):
    """gtsam.PreintegrationCombinedParams: PreintegrationParams plus the continuous-time bias random walk.  STATED DEVIATION:
    the uncertainty of the bias estimate used during preintegration (biasAccOmegaInt in gtsam 4.0 / 4.1, biasAccOmegaInit in
    4.2) is not modelled; its default here is zero (upstream 4.0: the identity) and its setters accept only zero."""

    def __init__(self, n_gravity):
        super().__init__(n_gravity)
        self.biasAccCovariance = np.eye(3)
        self.biasOmegaCovariance = np.eye(3)
        self.biasAccOmegaInt = np.zeros((6, 6))

    @staticmethod
    def MakeSharedU(g=9.81):
        return PreintegrationCombinedParams([0.0, 0.0, -float(g)])

    @staticmethod
    def MakeSharedD(g=9.81):
        return PreintegrationCombinedParams([0.0, 0.0, float(g)])

    def setBiasAccCovariance(self, c):
        self.biasAccCovariance = np.asarray(c, dtype=float)

    def setBiasOmegaCovariance(self, c):
        self.biasOmegaCovariance = np.asarray(c, dtype=float)

    def _set_bias_init(self, c, setter):
        c = np.asarray(c, dtype=float)
        if c.shape != (6, 6):
            raise RuntimeError(f"{setter}: a 6 x 6 matrix is expected, not an array of shape {c.shape}")
        if c.any():
            raise NotImplementedError(f"{setter}: the uncertainty of the bias estimate used during preintegration is not "
                                      "modelled by the combined preintegration; only the all-zero matrix is accepted")
        self.biasAccOmegaInt = np.zeros((6, 6))

    def setBiasAccOmegaInt(self, c):                                     # gtsam 4.0 / 4.1
        self._set_bias_init(c, "setBiasAccOmegaInt")

    def setBiasAccOmegaInit(self, c):                                    # gtsam 4.2
        self._set_bias_init(c, "setBiasAccOmegaInit")


class PreintegratedCombinedMeasurements(PreintegratedImuMeasurements):
    """gtsam.PreintegratedCombinedMeasurements(params, bias): the preintegration of PreintegratedImuMeasurements with the bias
    random walk of the same interval; preintMeasCov() is 15 x 15 in the error order (theta, p, v, b_a, b_g) (imu.py)."""

    def __init__(self, params: PreintegrationCombinedParams, bias: Optional[_ConstantBias] = None):
        from .imu import CombinedPreintegrator
        if not isinstance(params, PreintegrationCombinedParams):
            raise RuntimeError("PreintegratedCombinedMeasurements needs PreintegrationCombinedParams")
        self.params, self.bias = params, bias or _ConstantBias()
        self._pre = CombinedPreintegrator(self.bias.vector(), params.accelerometerCovariance, params.gyroscopeCovariance,
                                          params.integrationCovariance, params.biasAccCovariance, params.biasOmegaCovariance)

    def preintMeasCov(self):
        return self._pre.cov15.copy()


class CombinedImuFactor(_Factor):
    """CombinedImuFactor(pose_i, vel_i, pose_j, vel_j, bias_i, bias_j, pim): the IMU measurement and the bias walk of one
    keyframe interval as ONE 15-row factor under the full covariance of pim (include/vus_combined_imu.h).  Like gtsam, the
    factor copies the preintegrated measurement at construction.  Its noise model is that covariance and nothing else."""

    def __init__(self, pose_i, vel_i, pose_j, vel_j, bias_i, bias_j, pim: PreintegratedCombinedMeasurements, model=None):
        super().__init__([pose_i, vel_i, pose_j, vel_j, bias_i, bias_j])
        if model is not None:
            self.cloneWithNewNoiseModel(model)
        if not isinstance(pim, PreintegratedCombinedMeasurements):
            raise RuntimeError("CombinedImuFactor needs PreintegratedCombinedMeasurements")
        if int(bias_i) == int(bias_j):
            raise NotImplementedError(f"CombinedImuFactor: bias_i and bias_j are both {symbol_shorthand.key_string(int(bias_i))} -- that is the "
                                      "shared-bias layout, where a bias cannot walk; give the factor B(i) and B(i+1), or use "
                                      "ImuFactor with the one shared bias")
        if pim._pre.dt <= 0.0:
            raise RuntimeError("CombinedImuFactor: the preintegrated interval is empty (no IMU sample between the keyframes)")
        if pim.params.use2ndOrderCoriolis or np.any(pim.params.omegaCoriolis != 0):
            raise NotImplementedError("Coriolis terms are not implemented (batch.py:186-187 disables them)")
        self.pim = pim._pre.packed()
        self.W = pim._pre.whitening().reshape(-1)
        self.cov = pim._pre.cov15.copy()
        self.gravity = np.asarray(pim.params.n_gravity, dtype=float).copy()

    def cloneWithNewNoiseModel(self, model):
        kind = "a robust noise model" if isinstance(model, _Robust) else "a replaced noise model"
        raise NotImplementedError(f"CombinedImuFactor: {kind} is not supported -- the factor whitens with the 15 x 15 covariance "
                                  "of its PreintegratedCombinedMeasurements")


class DvlVelocityFactor(_Factor):
    """EXTENSION replacing the reference's DVL gtsam.CustomFactor (batch.py:196-250): same residual
    e = R_i * m - v_i on keys (V(i), X(i)), with the correct Jacobians (the callback of the reference returns
    3x3 Jacobians for a 6-dof Pose3 key, which no solver can use: SURVEY.md D7).
    DvlVelocityFactor(noiseModel, V(i), X(i), measured_body_velocity)."""

    def __init__(self, model: _NoiseModel, velKey: int, poseKey: int, measured):
        super().__init__([velKey, poseKey])
        _refuse_full(model, "DvlVelocityFactor")
        _refuse_robust(model, "DvlVelocityFactor")
        if model.dim() != 3 or not model.is_isotropic():
            raise NotImplementedError("DvlVelocityFactor needs an isotropic 3-dimensional noise model (batch.py:98)")
        self._model = model
        self.measured = np.asarray(measured, dtype=float).reshape(3).copy()


class CustomFactor(_Factor):
    def __init__(self, model: _NoiseModel, keys: Sequence[int], error_function: Callable):       # batch.py:245-249
        super().__init__(keys)
        self._model, self._fn = model, error_function


class HessianFactor(_Factor):
    """gtsam.HessianFactor(js, Gs, gs, f): upstream's n-way constructor.  `Gs` are the upper-triangle blocks G11, G12, ..,
    G1n, G22, .. in row-major order, `gs` one vector per key, and the error is 0.5 (f - 2 x^T g + x^T G x): upstream's g is
    MINUS the gradient at x = 0.  The conversion happens once, here: the factor keeps the dense symmetric G, the gradient
    -g and the constant f / 2, which is what include/vus_fixed_lag.h takes."""

    def __init__(self, js, Gs, gs, f):
        super().__init__(js)
        n = len(self._keys)
        gs = [np.asarray(g, dtype=float).reshape(-1) for g in gs]
        Gs = [np.asarray(G, dtype=float) for G in Gs]
        if len(gs) != n or len(Gs) != n * (n + 1) // 2:
            raise RuntimeError(f"HessianFactor: {n} keys need {n} vectors and {n * (n + 1) // 2} upper-triangle blocks, not "
                               f"{len(gs)} and {len(Gs)}")
        if len(set(self._keys)) != n:
            raise RuntimeError("HessianFactor: a key appears twice")
        dims = [len(g) for g in gs]
        off = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        G = np.zeros((off[-1], off[-1]))
        it = iter(Gs)
        for a in range(n):
            for b in range(a, n):
                blk = next(it)
                if blk.shape != (dims[a], dims[b]):
                    raise RuntimeError(f"HessianFactor: block ({a}, {b}) is {blk.shape}, ({dims[a]}, {dims[b]}) is expected")
                G[off[a]:off[a + 1], off[b]:off[b + 1]] = blk
                if b > a:
                    G[off[b]:off[b + 1], off[a]:off[a + 1]] = blk.T
        self._dims, self._G = dims, G
        self._grad, self._c = -np.concatenate(gs) if n else np.zeros(0), 0.5 * float(f)

    @classmethod
    def _from_dense(cls, keys, H, grad, c, dim=6, dims=None):
        """The factor over `keys` (`dim` values each, or `dims` per key) with information H, GRADIENT grad and constant c."""
        self = cls.__new__(cls)
        _Factor.__init__(self, keys)
        self._dims = [dim] * len(self._keys) if dims is None else [int(d) for d in dims]
        n = sum(self._dims)
        self._G = np.array(H, dtype=float).reshape(n, n)
        self._grad, self._c = np.array(grad, dtype=float).reshape(n), float(c)
        return self

    def information(self):
        return self._G.copy()

    def linearTerm(self):
        """upstream's g = minus the gradient"""
        return -self._grad

    def constantTerm(self):
        return 2.0 * self._c

    def error(self, delta):
        """0.5 (f - 2 x^T g + x^T G x) at the stacked vector x, the keys in the factor's order."""
        x = np.asarray(delta, dtype=float).reshape(-1)
        return float(self._c + self._grad @ x + 0.5 * x @ self._G @ x)


class LinearContainerFactor(_Factor):
    """gtsam.LinearContainerFactor(factor, linearizationPoint): a linear factor held in a nonlinear graph, evaluated at
    delta = Local(linearizationPoint, values).  Served for a HessianFactor over Pose3 keys that are consecutive in the
    graph's sorted pose table, at most one per graph: the optimizer lowers it to a ba.WindowPrior (the dense prior a
    fixed-lag smoother leaves of marginalised keyframes).  A second shape is served next to it: X(i), V(i) and B(i) of
    consecutive keyframes with blocks of 6, 3 and 6 values, lowered to a ba.NavWindowPrior in the per-keyframe-bias layout.
    Anything else is refused with the reason when the graph is packed."""

    def __init__(self, factor, linearizationPoint):
        if not isinstance(factor, HessianFactor):
            raise NotImplementedError(f"LinearContainerFactor holds a HessianFactor here, not a {type(factor).__name__}")
        super().__init__(factor.keys())
        self._factor = factor
        self._point = Values()
        for k in self._keys:
            if not linearizationPoint.exists(k):
                raise RuntimeError(f"Attempting to at the key \"{symbol_shorthand.key_string(k)}\", which does not exist in the Values.")
            self._point.insert(k, linearizationPoint._at(k, object, "at"))

    def factor(self):
        return self._factor

    def linearizationPoint(self):
        return self._point

    def _is_inertial(self):
        """The second served shape: X(i), V(i), B(i) keys -- at least an X and one of the others, and nothing else."""
        chars = {symbol_shorthand.symbolChr(k) for k in self._keys}
        return "x" in chars and len(chars) > 1 and chars <= {"x", "v", "b"}

    def _nav_window(self, pose_keys):
        """The inertial shape lowered to a ba.NavWindowPrior, as a dict (first, x0 [m, 12], v0 [m, 3], b0 [m, 6], H, g, c)
        over the sorted Pose3 keys `pose_keys` of a graph's Values: X(i), V(i) and B(i) of consecutive keyframes with blocks
        of 6, 3 and 6 values, the keys in any order, the linearisation point a Pose3, a 3-vector and a ConstantBias per
        keyframe.  Anything in between is refused with the reason."""
        f, sym = self._factor, symbol_shorthand
        name = sym.key_string
        want = {"x": (6, "a Pose3"), "v": (3, "a 3-vector"), "b": (6, "an imuBias.ConstantBias")}
        off = np.concatenate([[0], np.cumsum(f._dims)]).astype(int)
        per = {}
        for pos, k in enumerate(self._keys):
            per.setdefault(sym.symbolIndex(k), {})[sym.symbolChr(k)] = pos
        for i in sorted(per):
            missing = [c for c in "xvb" if c not in per[i]]
            if missing:
                raise NotImplementedError(
                    f"LinearContainerFactor: keyframe {i} has {', '.join(name(self._keys[p]) for p in per[i].values())} but not "
                    f"{', '.join(name(sym.symbol(c, i)) for c in missing)}; an inertial prior covers X(i), V(i) and B(i) of "
                    "every keyframe it touches")
            for c, pos in per[i].items():
                k, (dim, what) = self._keys[pos], want[c]
                if f._dims[pos] != dim:
                    raise NotImplementedError(f"LinearContainerFactor: key {name(k)} has a block of {f._dims[pos]} values, {dim} "
                                              f"are expected ({what})")
                val = self._point._at(k, object, "at")
                ok = (isinstance(val, Pose3) if c == "x" else isinstance(val, _ConstantBias) if c == "b"
                      else isinstance(val, np.ndarray) and val.size == 3)
                if not ok:
                    raise NotImplementedError(f"LinearContainerFactor: key {name(k)} is not {what} in the linearisation point")
        kfs = sorted(per)
        xkeys = np.asarray([sym.symbol("x", i) for i in kfs], dtype=np.int64)
        idx = np.searchsorted(pose_keys, xkeys)
        for k, j in zip(xkeys.tolist(), idx.tolist()):
            if j >= len(pose_keys) or pose_keys[j] != k:
                raise RuntimeError(f"Attempting to at the key \"{name(k)}\", which does not exist in the Values.")
        if len(idx) > 1 and bool((np.diff(idx) != 1).any()):
            raise NotImplementedError("LinearContainerFactor: its keyframes " + ", ".join(name(k) for k in xkeys.tolist())
                                      + " are not consecutive among the Pose3 keys of the Values")
        rows = np.concatenate([np.arange(off[per[i][c]], off[per[i][c] + 1]) for i in kfs for c in "xvb"])
        at = lambda c: [self._point._at(sym.symbol(c, i), object, "at") for i in kfs]
        return dict(first=int(idx[0]), x0=self._point.pose3_block(xkeys),
                    v0=np.stack([np.asarray(v, dtype=float).reshape(3) for v in at("v")]),
                    b0=np.stack([b.vector() for b in at("b")]), H=f._G[np.ix_(rows, rows)], g=f._grad[rows], c=f._c)

    def _window(self, pose_keys):
        """(first, x0 [m, 12], H, g, c) over the sorted Pose3 keys `pose_keys` of a graph's Values, or the refusal."""
        f = self._factor
        if not self._keys:
            raise NotImplementedError("LinearContainerFactor: a factor without keys")
        if any(d != 6 for d in f._dims):
            raise NotImplementedError("LinearContainerFactor: every key must be a Pose3 (6 values), the factor has blocks of "
                                      f"{sorted(set(f._dims))}")
        name = symbol_shorthand.key_string
        for k in self._keys:
            if not isinstance(self._point._at(k, object, "at"), Pose3):
                raise NotImplementedError(f"LinearContainerFactor: key {name(k)} is not a Pose3 in the linearisation point; priors "
                                          "tied to landmarks are not supported")
        keys = np.asarray(self._keys, dtype=np.int64)
        order = np.argsort(keys)
        idx = np.searchsorted(pose_keys, keys[order])
        for k, j in zip(keys[order].tolist(), idx.tolist()):
            if j >= len(pose_keys) or pose_keys[j] != k:
                raise RuntimeError(f"Attempting to at the key \"{name(k)}\", which does not exist in the Values.")
        if len(idx) > 1 and bool((np.diff(idx) != 1).any()):
            raise NotImplementedError("LinearContainerFactor: its keys " + ", ".join(name(k) for k in keys[order].tolist())
                                      + " are not consecutive among the Pose3 keys of the Values")
        rows = (6 * order[:, None] + np.arange(6)[None, :]).reshape(-1)       # the factor's rows in sorted key order
        x0 = self._point.pose3_block(keys[order])
        return int(idx[0]), x0, f._G[np.ix_(rows, rows)], f._grad[rows], f._c


class NavState:
    def __init__(self, pose=None, velocity=None):
        self._pose, self._v = pose or Pose3(), np.zeros(3) if velocity is None else np.asarray(velocity, float)


class ConstantTwistScenario:
    """Imported by batch.py:19-25 and never used; only the name has to exist for the import line."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("ConstantTwistScenario is imported but unused by batch.py; not part of the hot path")


class PinholeCameraCal3_S2:
    """gtsam.PinholeCameraCal3_S2(pose, K), host-only: for initialising landmarks (backproject) and synthesising
    measurements (project); the factors' arithmetic runs on the GPU.  project() is the prediction of
    GenericProjectionFactorCal3_S2 for the camera pose (pose o body_P_sensor of the factor)."""

    def __init__(self, pose: Optional[Pose3] = None, K: Optional[Cal3_S2] = None):
        self._pose = Pose3() if pose is None else Pose3(pose)
        self._K = Cal3_S2() if K is None else K
        if not isinstance(self._K, Cal3_S2):
            raise RuntimeError("PinholeCameraCal3_S2 needs a Cal3_S2 calibration")

    def pose(self):
        return Pose3(self._pose)

    def calibration(self):
        return self._K

    def project(self, point):
        """Point2 (u, v) of a world point; RuntimeError (gtsam's CheiralityException) at or behind the camera."""
        q = self._pose.transformTo(np.asarray(point, dtype=float).reshape(3))
        if q[2] <= 0.0:
            raise RuntimeError("CheiralityException: the point is behind the camera")
        fx, fy, s, u0, v0 = self._K._v
        return np.array([u0 + fx * q[0] / q[2] + s * q[1] / q[2], v0 + fy * q[1] / q[2]])

    def backproject(self, p, depth):
        """The world point at `depth` along the ray of pixel p."""
        fx, fy, s, u0, v0 = self._K._v
        p = np.asarray(p, dtype=float).reshape(2)
        yn = (p[1] - v0) / fy
        xn = (p[0] - u0 - s * yn) / fx
        return self._pose.transformFrom(float(depth) * np.array([xn, yn, 1.0]))


class ISAM2:
    """Constructed but never used by batch.py (batch.py:79); iSAM2 is out of scope."""

    def __init__(self, *args, **kwargs):
        pass

    def update(self, *args, **kwargs):
        raise NotImplementedError("ISAM2 is outside the hot path (isam.py is declared broken: README.md:40-41)")


# ---------------------------------------------------------------------------------------------
# containers
class _ValueBlock:
    """Array-backed run of same-typed variables (EXTENSION, see Values.insert_point3_block): keys ascending,
    data [n,3] (Point3) or [n,12] (Pose3 as row-major R then t)."""
    __slots__ = ("kind", "keys", "data")

    def __init__(self, kind, keys, data):
        self.kind, self.keys, self.data = kind, keys, data

    def find(self, keys):
        """(position, found) of every key of the int64 array `keys` in this block."""
        if len(self.keys) == 0:
            return np.zeros(len(keys), np.int64), np.zeros(len(keys), bool)
        pos = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return pos, self.keys[pos] == keys


class _Slot:
    """Dictionary entry of a variable whose value lives in one of the Values' growing columnar stores."""
    __slots__ = ("kind", "row")

    def __init__(self, kind, row):
        self.kind, self.row = kind, row


_WIDTH = {"point3": 3, "pose3": 12}


class _Column:
    """Growing columnar store of same-typed variables inserted ONE BY ONE (the way batch.py:283-298 inserts them):
    keys and values are appended to flat C arrays at insertion time, so that packing a graph for the GPU, and writing
    its result back, never loops over the variables in Python.  A sorted view (keys ascending -> row) is built lazily
    and dropped by every insertion / erasure."""
    __slots__ = ("kind", "width", "keys", "data", "dead", "_view")

    def __init__(self, kind, other: Optional["_Column"] = None):
        self.kind, self.width = kind, _WIDTH[kind]
        self.keys = array("q", other.keys) if other is not None else array("q")
        self.data = array("d", other.data) if other is not None else array("d")
        self.dead = other.dead if other is not None else 0
        self._view = None

    def append(self, key, flat):
        self.keys.append(key)
        self.data.extend(flat)
        self._view = None
        return len(self.keys) - 1

    def row(self, r):
        w = self.width
        return np.array(self.data[w * r:w * (r + 1)])

    def set_row(self, r, flat):
        w = self.width
        self.data[w * r:w * (r + 1)] = array("d", flat)

    def kill(self, r):
        self.keys[r] = -1              # keys are symbols (chr << 56 | index) or plain non-negative integers
        self.dead += 1
        self._view = None

    def arrays(self):
        """(keys int64 [n], data f64 [n, width]) VIEWS of the live storage.  While such a view is alive the stores cannot
        grow (array.append raises BufferError), so no view ever leaves this class: callers get copies (take) and
        write through put."""
        k = np.frombuffer(self.keys, dtype=np.int64) if len(self.keys) else np.zeros(0, np.int64)
        d = (np.frombuffer(self.data, dtype=np.float64) if len(self.data) else np.zeros(0)).reshape(-1, self.width)
        return k, d

    def take(self, rows):
        """Copy of the given rows [m, width]."""
        return self.arrays()[1][rows]

    def put(self, rows, values):
        self.arrays()[1][rows] = values

    def view(self):
        """(sorted live keys, their rows)."""
        if self._view is None:
            k, _ = self.arrays()
            order = np.argsort(k, kind="stable")
            if self.dead:
                order = order[k[order] >= 0]
            self._view = (k[order], order)
        return self._view

    def find(self, keys):
        sk, rows = self.view()
        if len(sk) == 0:
            return np.zeros(len(keys), np.int64), np.zeros(len(keys), bool)
        pos = np.minimum(np.searchsorted(sk, keys), len(sk) - 1)
        return rows[pos], sk[pos] == keys

    def __len__(self):
        return len(self.keys) - self.dead


class Values:
    """gtsam.Values.  Storage is columnar from the moment of insertion: 3-vectors (Point3 landmarks, velocities) and
    Pose3 values inserted one by one (batch.py:283-298) are appended to growing flat arrays (`_Column`), whole runs
    inserted through the bulk EXTENSION methods are kept as arrays (`_ValueBlock`); only values of other types
    (imuBias.ConstantBias, vectors of other sizes, Rot3) are held as objects.  Packing a 50 000-landmark graph for the
    GPU and reading its result back therefore involve no per-variable Python work."""

    def __init__(self, other: Optional["Values"] = None):
        self._d: Dict[int, object] = dict(other._d) if other is not None else {}
        self._blk: List[_ValueBlock] = ([_ValueBlock(b.kind, b.keys, b.data.copy()) for b in other._blk]
                                        if other is not None else [])
        self._col = {k: _Column(k, other._col[k] if other is not None else None) for k in _WIDTH}

    # -- block helpers ------------------------------------------------------------------------------
    def _find_block(self, key):
        for b in self._blk:
            n = len(b.keys)
            if n:
                i = int(np.searchsorted(b.keys, key))
                if i < n and b.keys[i] == key:
                    return b, i
        return None, -1

    def _insert_block(self, kind, keys, data, width):
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        data = np.array(data, dtype=float).reshape(-1, width)
        if len(keys) != len(data):
            raise RuntimeError("Values: keys and values differ in length")
        order = np.argsort(keys, kind="stable")
        keys, data = keys[order], data[order]
        dup = len(keys) > 1 and bool((keys[1:] == keys[:-1]).any())
        if not dup and self._d:
            dup = any(int(k) in self._d for k in keys.tolist()) if len(keys) < len(self._d) else \
                bool(np.isin(np.fromiter(self._d.keys(), np.int64, len(self._d)), keys).any())
        for b in self._blk:
            dup = dup or bool(b.find(keys)[1].any())
        if dup:
            raise RuntimeError("Attempting to add a key-value pair with a key which already exists in the Values.")
        self._blk.append(_ValueBlock(kind, keys, data))

    def insert_point3_block(self, keys, points):
        """EXTENSION: vectorised `for k, p in zip(keys, points): insert(k, p)` (batch.py:297-298)."""
        self._insert_block("point3", keys, points, 3)

    def insert_pose3_block(self, keys, flat12):
        """EXTENSION: bulk insertion of Pose3 values given as [n,12] rows (row-major R, then t)."""
        self._insert_block("pose3", keys, flat12, 12)

    insert_points = insert_point3_block

    def _stores(self, kind):
        """Every array-backed store that can hold variables of `kind`: (find(keys) -> (rows, hit), take(rows) -> copy,
        put(rows, values), kind).  No view of a growing column is handed out (see _Column.arrays)."""
        for b in self._blk:
            yield b.find, b.data.__getitem__, b.data.__setitem__, b.kind
        for c in self._col.values():
            if len(c):
                yield c.find, c.take, c.put, c.kind

    def _rows(self, kind, keys, what):
        """[n,w] array of the variables `keys` (int64 array) of the given kind; raises like gtsam's at*()."""
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        out = np.empty((len(keys), _WIDTH[kind]))
        todo = np.ones(len(keys), bool)
        for find, take, _, k in self._stores(kind):
            pos, hit = find(keys)
            hit &= todo
            if hit.any():
                if k != kind:
                    bad = int(keys[np.nonzero(hit)[0][0]])
                    raise RuntimeError(f"Values: key \"{symbol_shorthand.key_string(bad)}\" does not hold what {what} asks for")
                out[hit] = take(pos[hit])
                todo &= ~hit
        for i in np.nonzero(todo)[0].tolist():      # what is left is absent, or an object of another type
            k = int(keys[i])
            if k not in self._d:
                raise RuntimeError(f"Attempting to at the key \"{symbol_shorthand.key_string(k)}\", "
                                   "which does not exist in the Values.")
            raise RuntimeError(f"Values: key \"{symbol_shorthand.key_string(k)}\" is not a "
                               f"{'Pose3' if kind == 'pose3' else 'Point3'}")
        return out

    def point3_block(self, keys):
        """EXTENSION: [n,3] array of the Point3 variables `keys` (bulk atPoint3)."""
        return self._rows("point3", keys, "atPoint3")

    def pose3_block(self, keys):
        """EXTENSION: [n,12] array (row-major R, then t) of the Pose3 variables `keys` (bulk atPose3)."""
        return self._rows("pose3", keys, "atPose3")

    def _pose3_table(self):
        """(sorted keys, [n,12]) of every Pose3 variable."""
        sk, rows = self._col["pose3"].view()
        ks, data = [sk], [self._col["pose3"].take(rows)]
        for b in self._blk:
            if b.kind == "pose3":
                ks.append(b.keys); data.append(b.data)
        keys, data = np.concatenate(ks), np.concatenate(data)
        order = np.argsort(keys, kind="stable")
        return keys[order], data[order]

    def _store_rows(self, kind, keys, rows):
        """Overwrite existing variables of `kind` (result write-back of the optimizer), vectorised."""
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        todo = np.ones(len(keys), bool)
        for find, _, put, k in self._stores(kind):
            if k != kind:
                continue
            pos, hit = find(keys)
            hit &= todo
            put(pos[hit], rows[hit])
            todo &= ~hit
        if todo.any():
            k = int(keys[np.nonzero(todo)[0][0]])
            raise RuntimeError(f"Values: key \"{symbol_shorthand.key_string(k)}\" is not a stored "
                               f"{'Pose3' if kind == 'pose3' else 'Point3'}")

    # -- gtsam API ---------------------------------------------------------------------------------
    def _put(self, key, v):
        if isinstance(v, Pose3):
            self._d[key] = _Slot("pose3", self._col["pose3"].append(key, v.flat12()))
        elif isinstance(v, np.ndarray) and v.size == 3:
            self._d[key] = _Slot("point3", self._col["point3"].append(key, v))
        else:
            self._d[key] = v

    def insert(self, key, value):                                        # batch.py:274,283-288,298
        key = int(key)
        if key in self._d or (self._blk and self._find_block(key)[0] is not None):
            raise RuntimeError(f"Attempting to add a key-value pair with key \"{symbol_shorthand.key_string(key)}\", "
                               "which already exists in the Values.")
        self._put(key, self._coerce(value))

    def update(self, key, value):
        key = int(key)
        v = self._coerce(value)
        b, i = self._find_block(key)
        held = b.kind if b is not None else None
        if b is None:
            if key not in self._d:
                raise RuntimeError(f"Requested to update a key-value pair with key \"{symbol_shorthand.key_string(key)}\", "
                                   "which does not exist in the Values.")
            cur = self._d[key]
            if not isinstance(cur, _Slot):       # an object-held value: replaced by whatever comes, as before
                del self._d[key]
                self._put(key, v)
                return
            held = cur.kind
        # gtsam refuses to change a variable's type through update(): same RuntimeError as _at() / _rows()
        ok = isinstance(v, Pose3) if held == "pose3" else (isinstance(v, np.ndarray) and v.size == 3)
        if not ok:
            raise RuntimeError(f"Values: key \"{symbol_shorthand.key_string(key)}\" holds a "
                               f"{'Pose3' if held == 'pose3' else 'Point3'}, not the {type(v).__name__} update() was given")
        flat = v.flat12() if held == "pose3" else v
        if b is not None:
            b.data[i] = flat
        else:
            self._col[held].set_row(self._d[key].row, flat)

    def insert_or_assign(self, key, value):
        if self.exists(key):
            self.update(key, value)
        else:
            self.insert(key, value)

    @staticmethod
    def _coerce(value):
        if isinstance(value, (Pose3, Rot3, _ConstantBias)):
            return value
        return np.asarray(value, dtype=float).reshape(-1).copy()

    def exists(self, key):                                               # batch.py:60,297
        key = int(key)
        return key in self._d or (bool(self._blk) and self._find_block(key)[0] is not None)

    def erase(self, key):
        key = int(key)
        b, i = self._find_block(key)
        if b is not None:
            b.keys, b.data = np.delete(b.keys, i), np.delete(b.data, i, axis=0)
            return
        if key not in self._d:
            raise RuntimeError(f"key \"{symbol_shorthand.key_string(key)}\" does not exist in the Values")
        cur = self._d.pop(key)
        if isinstance(cur, _Slot):
            self._col[cur.kind].kill(cur.row)

    def _at(self, key, kind, name):
        key = int(key)
        if key in self._d:
            v = self._d[key]
            if isinstance(v, _Slot):
                r = self._col[v.kind].row(v.row)
                v = Pose3.from_flat12(r) if v.kind == "pose3" else r
        else:
            b, i = self._find_block(key)
            if b is None:
                raise RuntimeError(f"Attempting to {name} the key \"{symbol_shorthand.key_string(key)}\", "
                                   "which does not exist in the Values.")
            v = Pose3.from_flat12(b.data[i]) if b.kind == "pose3" else b.data[i].copy()
        if not isinstance(v, kind):
            raise RuntimeError(f"Values: key \"{symbol_shorthand.key_string(key)}\" holds a "
                               f"{type(v).__name__}, not what {name} asks for")
        return v

    def atPose3(self, key):                                              # batch.py:61,211
        return self._at(key, Pose3, "atPose3")

    def atVector(self, key):                                             # batch.py:210
        return self._at(key, np.ndarray, "atVector").copy()

    def atPoint3(self, key):
        v = self._at(key, np.ndarray, "atPoint3")
        if v.size != 3:
            raise RuntimeError("atPoint3: value is not a 3-vector")
        return v.copy()

    def atConstantBias(self, key):
        return self._at(key, _ConstantBias, "atConstantBias")

    def keys(self):
        ks = list(self._d)
        for b in self._blk:
            ks.extend(b.keys.tolist())
        return sorted(ks)

    def size(self):
        return len(self._d) + sum(len(b.keys) for b in self._blk)

    def __len__(self):
        return self.size()


class NonlinearFactorGraph:
    """gtsam.NonlinearFactorGraph.  GenericStereoFactor3D factors are ALSO recorded column-wise at the moment they are
    added (measurement, pose key, landmark key appended to flat arrays), so that the optimizer packs a graph of two
    million such objects (batch.py:300-305 pushes one per observation) without visiting them again."""

    def __init__(self):
        self._factors: List[_Factor] = []
        self._other: List[_Factor] = []          # everything that is not a single GenericStereoFactor3D
        self._st_meas, self._st_pk, self._st_lk = array("d"), array("q"), array("q")
        self._st_model = self._st_K = self._st_sensor = None     # the one noise model / calibration / extrinsic the stereo factors share ...
        self._st_mixed = False                   # ... or the fact that they do not (refused at optimize())
        # single GenericProjectionFactorCal3_S2 factors, column-wise in the same way: (u, v), pose key, point key
        self._mo_meas, self._mo_pk, self._mo_lk = array("d"), array("q"), array("q")
        self._mo_model = self._mo_K = self._mo_sensor = None
        self._mo_mixed = False

    def _record(self, factor):
        self._factors.append(factor)
        if type(factor) is GenericStereoFactor3D:
            m, K, S = factor._model, factor._K, factor._sensor
            if self._st_model is None:
                self._st_model, self._st_K, self._st_sensor = m, K, S
            elif (m is not self._st_model and _stereo_model_key(m) != _stereo_model_key(self._st_model)) or \
                    (K is not self._st_K and not K.equals(self._st_K)) or \
                    (S is not self._st_sensor and not _same_sensor(S, self._st_sensor)):
                self._st_mixed = True
            self._st_meas.extend(factor._measured._m)
            self._st_pk.append(factor._keys[0])
            self._st_lk.append(factor._keys[1])
        elif type(factor) is GenericProjectionFactorCal3_S2:
            m, K, S = factor._model, factor._K, factor._sensor
            if self._mo_model is None:
                self._mo_model, self._mo_K, self._mo_sensor = m, K, S
            elif (m is not self._mo_model and _stereo_model_key(m) != _stereo_model_key(self._mo_model)) or \
                    (K is not self._mo_K and not K.equals(self._mo_K)) or \
                    (S is not self._mo_sensor and not _same_sensor(S, self._mo_sensor)):
                self._mo_mixed = True
            self._mo_meas.extend(factor._measured)
            self._mo_pk.append(factor._keys[0])
            self._mo_lk.append(factor._keys[1])
        else:
            self._other.append(factor)

    def add(self, factor):                                               # batch.py:281-282
        self._record(factor)

    def push_back(self, factor):                                         # batch.py:291,292,305
        self._record(factor)

    def _stereo_columns(self):
        """(meas [n,3], pose keys [n], landmark keys [n], model, K, mixed) of the single stereo factors, in graph order."""
        n = len(self._st_pk)
        if n == 0:
            return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, False
        # copies (46 MB at two million factors, ~10 ms): a numpy VIEW of the growing arrays would pin their buffers and
        # make the next push_back fail with BufferError
        return (np.frombuffer(self._st_meas, dtype=np.float64).reshape(n, 3).copy(),
                np.frombuffer(self._st_pk, dtype=np.int64).copy(), np.frombuffer(self._st_lk, dtype=np.int64).copy(),
                self._st_model, self._st_K, self._st_mixed)

    def _mono_columns(self):
        """(meas [n,2], pose keys [n], point keys [n], model, K, mixed) of the single projection factors, in graph order."""
        n = len(self._mo_pk)
        if n == 0:
            return np.zeros((0, 2)), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, False
        return (np.frombuffer(self._mo_meas, dtype=np.float64).reshape(n, 2).copy(),
                np.frombuffer(self._mo_pk, dtype=np.int64).copy(), np.frombuffer(self._mo_lk, dtype=np.int64).copy(),
                self._mo_model, self._mo_K, self._mo_mixed)

    def size(self):
        return len(self._factors)

    def nrFactors(self):
        blocks = (StereoFactorBlock, ProjectionFactorBlock)
        return sum(f.size() if isinstance(f, blocks) else 1 for f in self._other) + len(self._st_pk) + len(self._mo_pk)

    def at(self, i):
        return self._factors[i]

    def keys(self):
        out = set()
        for f in self._other:
            out.update(f.keys())
        out.update(self._st_pk.tolist())
        out.update(self._st_lk.tolist())
        out.update(self._mo_pk.tolist())
        out.update(self._mo_lk.tolist())
        return sorted(out)

    def error(self, values: Values) -> float:
        """0.5 * sum of squared whitened residuals (sum of rho(d) for stereo factors under a noiseModel.Robust),
        evaluated on the GPU."""
        from .optimizer import graph_error
        return graph_error(self, values)

    def saveGraph(self, path, values=None):                              # batch.py:338
        """Graphviz DOT of the factor graph (variables as circles, factors as dots)."""
        ks = self.keys()
        with open(path, "w") as f:
            f.write("graph {\n  size=\"5,5\";\n\n")
            for k in ks:
                f.write(f"  var{k}[label=\"{symbol_shorthand.key_string(k)}\"];\n")
            f.write("\n")
            n = 0
            for fac in self._factors:
                if isinstance(fac, (StereoFactorBlock, ProjectionFactorBlock)):
                    for pk, lk in zip(fac.pose_keys.tolist(), fac.landmark_keys.tolist()):
                        f.write(f"  factor{n}[label=\"\", shape=point];\n  var{pk}--factor{n};\n  var{lk}--factor{n};\n")
                        n += 1
                    continue
                f.write(f"  factor{n}[label=\"\", shape=point];\n")
                for k in fac.keys():
                    f.write(f"  var{k}--factor{n};\n")
                n += 1
            f.write("}\n")


from .optimizer import LevenbergMarquardtParams, LevenbergMarquardtOptimizer  # noqa: E402
from .marginals import Marginals, JointMarginal, KeyVector, IndeterminantLinearSystemException  # noqa: E402
