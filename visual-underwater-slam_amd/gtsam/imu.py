"""IMU preintegration on the host, as GTSAM does it inside PreintegratedImuMeasurements
(/root/reference/batch.py:90-92,178-193,289-293 use it through pybind).  Restated from Forster et al.,
"On-Manifold Preintegration for Real-Time Visual-Inertial Odometry" (TRO 2017); O(#IMU samples) work at
graph-build time, not on the hot path.  The packed record layout (148 doubles) is shared with the
kernels (include/vus.h, vus_nav_factors.imu_pim) and with the oracle (oracle/vus_oracle_nav.c PIM_*)."""
import numpy as np

PIM_DT, PIM_DR, PIM_DP, PIM_DV = 0, 1, 10, 13
PIM_DR_DBG, PIM_DP_DBA, PIM_DP_DBG, PIM_DV_DBA, PIM_DV_DBG = 16, 25, 34, 43, 52
PIM_BIAS, PIM_COV, PIM_DOUBLES = 61, 67, 148


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_expmap(w):
    th2 = float(w @ w)
    W = skew(w)
    if th2 <= np.finfo(float).eps:
        return np.eye(3) + W
    th = np.sqrt(th2)
    return np.eye(3) + np.sin(th) / th * W + 2.0 * np.sin(0.5 * th) ** 2 / th2 * (W @ W)


def so3_jr(w):
    th2 = float(w @ w)
    W = skew(w)
    if th2 < 1e-10:
        a, b = 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = np.sqrt(th2)
        a, b = 2.0 * np.sin(0.5 * th) ** 2 / th2, (th - np.sin(th)) / (th2 * th)
    return np.eye(3) - a * W + b * (W @ W)


class Preintegrator:
    """State of one preintegration interval; integrate() consumes one (acc, gyro, dt) sample.

    The samples are BUFFERED and integrated by the library's host function vus_imu_preintegrate (C++, like GTSAM's own
    integrateMeasurement) the next time the state is read: a keyframe interval of 40 samples is one native call instead
    of 40 rounds of small numpy products (78 of the 92 ms of the 50-keyframe end-to-end sequence).  ReferencePreintegrator
    below is the numpy restatement the native function is tested against (and through it against the oracle)."""

    def __init__(self, bias_hat, acc_cov, gyro_cov, int_cov):
        self.bias_hat = np.asarray(bias_hat, dtype=float).reshape(6).copy()
        self.acc_cov, self.gyro_cov, self.int_cov = (np.ascontiguousarray(np.asarray(c, dtype=float).reshape(3, 3))
                                                     for c in (acc_cov, gyro_cov, int_cov))
        self.reset()

    def reset(self):
        self._rec = np.zeros(PIM_DOUBLES)
        self._rec[PIM_DR:PIM_DR + 9] = np.eye(3).reshape(-1)
        self._rec[PIM_BIAS:PIM_BIAS + 6] = self.bias_hat
        self._pending = []

    def integrate(self, acc, gyro, dt):
        dt = float(dt)
        if not dt > 0.0:
            raise ValueError(f"integrate: dt={dt} is not positive")
        a, w = np.asarray(acc, dtype=float).reshape(3), np.asarray(gyro, dtype=float).reshape(3)
        self._pending.append((a[0], a[1], a[2], w[0], w[1], w[2], dt))

    def _flush(self, whiten=None):
        if not self._pending and whiten is None:
            return
        from .. import _lib
        smp = np.ascontiguousarray(np.array(self._pending, dtype=np.float64).reshape(-1, 7))
        _lib.call("vus_imu_preintegrate", self._rec.ctypes.data, smp.ctypes.data, len(smp), self.acc_cov.ctypes.data,
                  self.gyro_cov.ctypes.data, self.int_cov.ctypes.data, None if whiten is None else whiten.ctypes.data)
        self._pending = []

    def _mat(self, off):
        self._flush()
        return self._rec[off:off + 9].reshape(3, 3).copy()

    dt = property(lambda self: (self._flush(), float(self._rec[PIM_DT]))[1])
    dR = property(lambda self: self._mat(PIM_DR))
    dP = property(lambda self: (self._flush(), self._rec[PIM_DP:PIM_DP + 3].copy())[1])
    dV = property(lambda self: (self._flush(), self._rec[PIM_DV:PIM_DV + 3].copy())[1])
    dR_dbg = property(lambda self: self._mat(PIM_DR_DBG))
    dP_dba = property(lambda self: self._mat(PIM_DP_DBA))
    dP_dbg = property(lambda self: self._mat(PIM_DP_DBG))
    dV_dba = property(lambda self: self._mat(PIM_DV_DBA))
    dV_dbg = property(lambda self: self._mat(PIM_DV_DBG))
    cov = property(lambda self: (self._flush(), self._rec[PIM_COV:PIM_COV + 81].reshape(9, 9).copy())[1])

    def packed(self):
        self._flush()
        return self._rec.copy()

    def whitening(self):
        """W = L^-1 with cov = L L^T: |W r|^2 = r^T cov^-1 r (what gtsam's Gaussian noise model does)."""
        W = np.zeros((9, 9))
        self._flush(whiten=W)
        return W


class ReferencePreintegrator:
    """The same recursion in numpy, sample by sample (tests: the native function against this, this against the oracle)."""

    def __init__(self, bias_hat, acc_cov, gyro_cov, int_cov):
        self.bias_hat = np.asarray(bias_hat, dtype=float).reshape(6).copy()
        self.acc_cov, self.gyro_cov, self.int_cov = (np.asarray(c, dtype=float).reshape(3, 3) for c in (acc_cov, gyro_cov, int_cov))
        self.reset()

    def reset(self):
        self.dt = 0.0
        self.dR, self.dP, self.dV = np.eye(3), np.zeros(3), np.zeros(3)
        self.dR_dbg = np.zeros((3, 3))
        self.dP_dba, self.dP_dbg = np.zeros((3, 3)), np.zeros((3, 3))
        self.dV_dba, self.dV_dbg = np.zeros((3, 3)), np.zeros((3, 3))
        self.cov = np.zeros((9, 9))

    def integrate(self, acc, gyro, dt):
        dt = float(dt)
        a = np.asarray(acc, dtype=float).reshape(3) - self.bias_hat[:3]
        w = np.asarray(gyro, dtype=float).reshape(3) - self.bias_hat[3:]
        dRinc, Jr = so3_expmap(w * dt), so3_jr(w * dt)
        RaX = self.dR @ skew(a)
        A = np.eye(9)
        A[0:3, 0:3] = dRinc.T
        A[3:6, 0:3] = -0.5 * dt * dt * RaX
        A[3:6, 6:9] = np.eye(3) * dt
        A[6:9, 0:3] = -dt * RaX
        B = np.zeros((9, 3)); C = np.zeros((9, 3))
        B[3:6] = 0.5 * dt * dt * self.dR
        B[6:9] = dt * self.dR
        C[0:3] = dt * Jr
        cov = A @ self.cov @ A.T + B @ (self.acc_cov / dt) @ B.T + C @ (self.gyro_cov / dt) @ C.T
        cov[3:6, 3:6] += self.int_cov * dt
        self.cov = cov
        t = RaX @ self.dR_dbg
        self.dP_dba = self.dP_dba + self.dV_dba * dt - 0.5 * dt * dt * self.dR
        self.dP_dbg = self.dP_dbg + self.dV_dbg * dt - 0.5 * dt * dt * t
        self.dV_dba = self.dV_dba - dt * self.dR
        self.dV_dbg = self.dV_dbg - dt * t
        self.dR_dbg = dRinc.T @ self.dR_dbg - dt * Jr
        Ra = self.dR @ a
        self.dP = self.dP + self.dV * dt + 0.5 * dt * dt * Ra
        self.dV = self.dV + dt * Ra
        self.dR = self.dR @ dRinc
        self.dt += dt

    def packed(self):
        p = np.zeros(PIM_DOUBLES)
        p[PIM_DT] = self.dt
        p[PIM_DR:PIM_DR + 9] = self.dR.reshape(-1)
        p[PIM_DP:PIM_DP + 3], p[PIM_DV:PIM_DV + 3] = self.dP, self.dV
        for off, M in ((PIM_DR_DBG, self.dR_dbg), (PIM_DP_DBA, self.dP_dba), (PIM_DP_DBG, self.dP_dbg),
                       (PIM_DV_DBA, self.dV_dba), (PIM_DV_DBG, self.dV_dbg)):
            p[off:off + 9] = M.reshape(-1)
        p[PIM_BIAS:PIM_BIAS + 6] = self.bias_hat
        p[PIM_COV:PIM_COV + 81] = self.cov.reshape(-1)
        return p

    def whitening(self):
        """W = L^-1 with cov = L L^T: |W r|^2 = r^T cov^-1 r (what gtsam's Gaussian noise model does)."""
        L = np.linalg.cholesky(self.cov)
        return np.linalg.solve(L, np.eye(9))


def residual_frame(cov15, dR):
    """T cov15 T^T with T = diag(I, dR^T, dR^T, I, I): the recursion carries the position and velocity errors in the frame of
    the EARLIER keyframe (as the 9 x 9 record does), the factor's residual has them in the frame of the LATER one (r_p =
    R_j^T (..), r_v = R_j^T (..), and R_j^T R_i = dR^T at the truth).  Under isotropic noise the 9 x 9 blocks do not tell the
    two apart; the cross blocks with the bias walk do, by the rotation of the interval (the Monte-Carlo test of
    tests/test_combined_imu_ref.py measures it)."""
    T = np.eye(15)
    T[3:6, 3:6] = T[6:9, 6:9] = np.asarray(dR).T
    return T @ cov15 @ T.T


class CombinedPreintegrator(Preintegrator):
    """Preintegrator with the bias random walk (gtsam.PreintegratedCombinedMeasurements): next to the 148-double record,
    whose means, bias Jacobians and 9 x 9 covariance are exactly Preintegrator's, a 15 x 15 covariance `cov15` in the error
    order (theta, p, v, b_a, b_g) of the measurement AND the bias drift of the interval, propagated by the library's host
    function vus_imu_preintegrate_combined (include/vus_combined_imu.h has the recursion).  The uncertainty of the bias
    estimate used for the preintegration (gtsam's biasAccOmegaInt / biasAccOmegaInit) is not modelled."""

    def __init__(self, bias_hat, acc_cov, gyro_cov, int_cov, bias_acc_cov, bias_omega_cov):
        self.bias_acc_cov, self.bias_omega_cov = (np.ascontiguousarray(np.asarray(c, dtype=float).reshape(3, 3))
                                                  for c in (bias_acc_cov, bias_omega_cov))
        super().__init__(bias_hat, acc_cov, gyro_cov, int_cov)

    def reset(self):
        super().reset()
        self._cov15 = np.zeros(225)

    def _flush(self, whiten=None):
        if not self._pending and whiten is None:
            return
        from .. import _lib
        smp = np.ascontiguousarray(np.array(self._pending, dtype=np.float64).reshape(-1, 7))
        self._pending = []              # whatever happens below, no sample is integrated twice
        try:
            _lib.call("vus_imu_preintegrate_combined", self._rec.ctypes.data, self._cov15.ctypes.data, smp.ctypes.data, len(smp),
                      self.acc_cov.ctypes.data, self.gyro_cov.ctypes.data, self.int_cov.ctypes.data,
                      self.bias_acc_cov.ctypes.data, self.bias_omega_cov.ctypes.data,
                      None if whiten is None else whiten.ctypes.data)
        except _lib.VusError as e:
            if "not positive definite" not in str(e):
                raise
            # the samples are integrated; only the factorisation was refused
            raise ValueError(_not_pd_reason(self.cov15, self.bias_acc_cov, self.bias_omega_cov)) from None

    cov15 = property(lambda self: (self._flush(), self._cov15.reshape(15, 15).copy())[1])

    def residual_cov(self):
        """The covariance of the factor's residual: cov15 with its p and v rows in the later keyframe's frame (residual_frame)"""
        return residual_frame(self.cov15, self.dR)

    def whitening(self):
        """W [15, 15] = L^-1 with residual_cov() = L L^T.  ValueError naming the parameter when it is not positive definite."""
        W = np.zeros((15, 15))
        self._flush(whiten=W)
        return W


def _not_pd_reason(cov15, bias_acc_cov, bias_omega_cov):
    """The sentence of the ValueError for a 15 x 15 covariance without a Cholesky factor: which parameter leaves it singular"""
    bad = [name for name, c in (("bias_acc_cov (setBiasAccCovariance)", bias_acc_cov),
                                ("bias_omega_cov (setBiasOmegaCovariance)", bias_omega_cov))
           if not (np.isfinite(c).all() and np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0.0)]
    if bad:
        return (f"the combined preintegrated covariance is not positive definite: {' and '.join(bad)} must be positive "
                "definite (a zero bias random walk is the ImuFactor + BetweenFactorConstantBias model, not this one)")
    if not np.diag(cov15)[:9].all():
        return ("the combined preintegrated covariance is not positive definite: the interval is empty or acc_cov / gyro_cov "
                "(setAccelerometerCovariance / setGyroscopeCovariance) leave a measurement row without noise")
    return "the combined preintegrated covariance is not positive definite"


class ReferenceCombinedPreintegrator(ReferencePreintegrator):
    """The same 15 x 15 recursion in numpy, sample by sample: Sigma <- F Sigma F^T + Q with F = [[A, G], [0, I]], A, B, C of
    ReferencePreintegrator.integrate, G = [B | C] (a bias error acts on the increments like the sensor noise of the same
    axis) and Q = the 9 x 9 noise plus bias_cov * dt on the bias blocks.  `cov` stays ReferencePreintegrator's."""

    def __init__(self, bias_hat, acc_cov, gyro_cov, int_cov, bias_acc_cov, bias_omega_cov):
        self.bias_acc_cov, self.bias_omega_cov = (np.asarray(c, dtype=float).reshape(3, 3) for c in (bias_acc_cov, bias_omega_cov))
        super().__init__(bias_hat, acc_cov, gyro_cov, int_cov)

    def reset(self):
        super().reset()
        self.cov15 = np.zeros((15, 15))

    def integrate(self, acc, gyro, dt):
        dt = float(dt)
        a = np.asarray(acc, dtype=float).reshape(3) - self.bias_hat[:3]
        w = np.asarray(gyro, dtype=float).reshape(3) - self.bias_hat[3:]
        dRinc, Jr = so3_expmap(w * dt), so3_jr(w * dt)
        RaX = self.dR @ skew(a)
        F = np.eye(15)
        F[0:3, 0:3] = dRinc.T
        F[3:6, 0:3] = -0.5 * dt * dt * RaX
        F[3:6, 6:9] = np.eye(3) * dt
        F[6:9, 0:3] = -dt * RaX
        B = np.zeros((9, 3)); C = np.zeros((9, 3))
        B[3:6] = 0.5 * dt * dt * self.dR
        B[6:9] = dt * self.dR
        C[0:3] = dt * Jr
        F[0:9, 9:12], F[0:9, 12:15] = B, C
        Q = np.zeros((15, 15))
        Q[:9, :9] = B @ (self.acc_cov / dt) @ B.T + C @ (self.gyro_cov / dt) @ C.T
        Q[3:6, 3:6] += self.int_cov * dt
        Q[9:12, 9:12], Q[12:15, 12:15] = self.bias_acc_cov * dt, self.bias_omega_cov * dt
        self.cov15 = F @ self.cov15 @ F.T + Q
        super().integrate(acc, gyro, dt)

    def residual_cov(self):
        return residual_frame(self.cov15, self.dR)

    def whitening(self):
        """W [15, 15] = L^-1 with residual_cov() = L L^T"""
        L = np.linalg.cholesky(self.residual_cov())
        return np.linalg.solve(L, np.eye(15))
