"""LevenbergMarquardtParams / LevenbergMarquardtOptimizer with gtsam's names and defaults
(/root/reference/batch.py:337), backed by the HIP bundle-adjustment kernels (../ba.py).

Host work here is graph -> structure-of-arrays packing (the vectorised form of batch.py:295-305);
every residual, Jacobian, linear solve and error is computed on the GPU.
"""
import math
from typing import List, Optional

import numpy as np

from . import symbol_shorthand as _sym


class LevenbergMarquardtParams:
    """gtsam.LevenbergMarquardtParams(): same defaults, same setter/getter names."""

    def __init__(self):
        self.lambdaInitial = 1e-5
        self.lambdaFactor = 10.0
        self.lambdaUpperBound = 1e5
        self.lambdaLowerBound = 0.0
        self.minModelFidelity = 1e-3
        self.diagonalDamping = False
        self.useFixedLambdaFactor = True
        self.maxIterations = 100
        self.relativeErrorTol = 1e-5
        self.absoluteErrorTol = 1e-5
        self.errorTol = 0.0
        self.verbosity = "SILENT"
        self.verbosityLM = "SILENT"
        self.longClosureSpan = None      # EXTENSION (setLongClosureSpan)

    # gtsam's accessor spelling
    def setlambdaInitial(self, v): self.lambdaInitial = float(v)
    def setlambdaFactor(self, v): self.lambdaFactor = float(v)
    def setlambdaUpperBound(self, v): self.lambdaUpperBound = float(v)
    def setlambdaLowerBound(self, v): self.lambdaLowerBound = float(v)
    def setDiagonalDamping(self, v): self.diagonalDamping = bool(v)
    def setUseFixedLambdaFactor(self, v): self.useFixedLambdaFactor = bool(v)
    def setMaxIterations(self, v): self.maxIterations = int(v)
    def setRelativeErrorTol(self, v): self.relativeErrorTol = float(v)
    def setAbsoluteErrorTol(self, v): self.absoluteErrorTol = float(v)
    def setErrorTol(self, v): self.errorTol = float(v)
    def setVerbosity(self, v): self.verbosity = str(v)
    def setVerbosityLM(self, v): self.verbosityLM = str(v)
    def setLongClosureSpan(self, m):
        """EXTENSION (not in gtsam): BetweenFactorPose3 whose keys lie more than m poses apart stay out of the band of the
        reduced camera system and enter every solve as a low-rank correction (ba.BetweenFactors(max_span=m)); None, the
        default, adds every between factor to the band, which widens to the longest of them."""
        self.longClosureSpan = None if m is None else int(m)
    def getLongClosureSpan(self): return self.longClosureSpan
    def getlambdaInitial(self): return self.lambdaInitial
    def getlambdaFactor(self): return self.lambdaFactor
    def getlambdaUpperBound(self): return self.lambdaUpperBound
    def getlambdaLowerBound(self): return self.lambdaLowerBound
    def getDiagonalDamping(self): return self.diagonalDamping
    def getMaxIterations(self): return self.maxIterations
    def getRelativeErrorTol(self): return self.relativeErrorTol
    def getAbsoluteErrorTol(self): return self.absoluteErrorTol
    def getErrorTol(self): return self.errorTol

    def _to_lm(self):
        from ..ba import LMParams
        return LMParams(self.lambdaInitial, self.lambdaFactor, self.lambdaUpperBound, self.lambdaLowerBound,
                        self.minModelFidelity, self.maxIterations, self.relativeErrorTol, self.absoluteErrorTol,
                        self.errorTol, self.diagonalDamping, self.useFixedLambdaFactor)


class _AuxPriors:
    """Vector variables constrained only by PriorFactorVector: they decouple from the camera system,
    so their damped step is closed-form per coordinate; kept on the host (O(#such variables))."""

    def __init__(self):
        self.keys: List[int] = []
        self.x: List[np.ndarray] = []
        self.prior: List[np.ndarray] = []
        self.w: List[np.ndarray] = []
        self._cand = None

    def add(self, key, x, prior, sigmas):
        self.keys.append(key); self.x.append(x.copy()); self.prior.append(prior.copy()); self.w.append(1.0 / sigmas)

    def error(self):
        return sum(0.5 * float(np.sum((w * (x - p)) ** 2)) for x, p, w in zip(self.x, self.prior, self.w))

    def try_lambda(self, lam):
        """returns (linearised error at the damped step, nonlinear error at the new values)"""
        lin, new, self._cand = 0.0, 0.0, []
        for x, p, w in zip(self.x, self.prior, self.w):
            r = w * (x - p)
            d = -(w * r) / (w * w + lam)
            self._cand.append(x + d)
            lin += 0.5 * float(np.sum((r + w * d) ** 2))
            new += 0.5 * float(np.sum((w * (x + d - p)) ** 2))
        return lin, new

    def accept(self):
        self.x = self._cand


_DVL_PROBES = None


def lower_reference_dvl_factor(f):
    """The reference builds its DVL factor as `gtsam.CustomFactor(Isotropic(3), [V(i), X(i)], partial(self.velocity_error,
    measurement))` with a 1x3 measurement (batch.py:241-250).  A Python callback per factor cannot run on the GPU, and
    the Jacobians that callback returns are ill-formed (3x3 for a 6-dof Pose3 key) -- but its RESIDUAL is
    well defined: e = R_i m - v_i (batch.py:213-228).  This function recognises exactly that factor, by shape AND by
    behaviour (the callback is evaluated at two probe states and must return R m - v to round-off), and returns the
    equivalent DvlVelocityFactor (same residual, analytic Jacobians de/dv = -I, de/dX = [-R [m]x, 0]); anything else
    returns None and stays refused."""
    import functools
    from . import CustomFactor, DvlVelocityFactor, Pose3, Rot3, Values
    global _DVL_PROBES
    if not isinstance(f, CustomFactor) or len(f._keys) != 2:
        return None
    kv, kx = f._keys
    if _sym.symbolChr(kv) != "v" or _sym.symbolChr(kx) != "x":
        return None
    model, fn = f._model, f._fn
    if model.dim() != 3 or not model.is_isotropic():
        return None
    if not isinstance(fn, functools.partial) or len(fn.args) != 1 or fn.keywords:
        return None
    m = np.asarray(fn.args[0], dtype=float)
    if m.shape not in ((1, 3), (3,)) or not np.isfinite(m).all():
        return None
    m3 = m.reshape(3)
    if _DVL_PROBES is None:
        _DVL_PROBES = [(Rot3.Expmap(np.array(w)), np.array(v)) for w, v in
                       (((0.3, -0.5, 0.8), (0.11, -0.23, 0.37)), ((-1.1, 0.4, 0.2), (-0.7, 0.05, 1.3)))]
    try:
        for R, v in _DVL_PROBES:
            probe = Values()
            probe.insert(kv, v)
            probe.insert(kx, Pose3(R, np.array([0.4, -0.9, 2.0])))
            e = np.asarray(fn(f, probe, None), dtype=float).reshape(-1)
            want = R.matrix() @ m3 - v
            if e.shape != (3,) or not np.allclose(e, want, rtol=0, atol=1e-12 * (1.0 + np.abs(want).max())):
                return None
    except Exception:                     # a callback that is not the reference's: refused by the caller
        return None
    return DvlVelocityFactor(model, kv, kx, m3)


def _pack_graph(graph, values, device=None, per_keyframe=False):
    """Factor graph + Values -> arrays for StereoBAProblem.  Raises on anything outside the built scope.
    `per_keyframe`: pack the inertial side with one bias per keyframe even where the graph alone would not say so (a single
    ImuFactor and no bias factor); a LinearContainerFactor over X, V, B keys forces the same.
    The per-observation key -> index mapping (a sort of every landmark key) runs on `device` with torch when one
    is given (2 M observations: ~3 ms on the GPU against ~0.3 s in numpy), else in numpy (CPU tests)."""
    from . import (GenericStereoFactor3D, StereoFactorBlock, PriorFactorPose3, PriorFactorVector, Pose3,
                   ImuFactor, CustomFactor, DvlVelocityFactor, _ConstantBias, PriorFactorConstantBias,
                   BetweenFactorConstantBias, BetweenFactorPose3, GenericProjectionFactorCal3_S2, ProjectionFactorBlock,
                   _PoseMeasFactor, LinearContainerFactor, CombinedImuFactor)
    container = None
    meas, pkeys, lkeys = [], [], []
    mono_n = []                     # per part of meas / pkeys / lkeys: 0 for a stereo part, its length for a mono part
    mono = dict(sigma=None, calib=None, loss=None, sensor=None)
    between_f, pose_meas_f = [], []
    imu_f, dvl_f, bias_f, cimu_f = [], [], [], []
    from . import _Robust
    from . import _same_sensor
    model_sigma, calib, loss, sensor = None, None, None, None
    prior_pose, prior_vec = [], []
    single_m, single_p, single_l = [], [], []

    def check_model(model, K, body_P_sensor):
        nonlocal model_sigma, calib, loss, sensor
        if not model.is_isotropic():
            raise NotImplementedError("stereo factors need an isotropic noise model (batch.py:118 uses Isotropic.Sigma(3, 10)), "
                                      "optionally wrapped in noiseModel.Robust")
        s = float(model.sigmas()[0])
        rob = model.robust() if isinstance(model, _Robust) else None
        lo = (rob.kind, rob.k) if rob is not None else None          # (VUS_LOSS_* kind, k) of a robust model
        if model_sigma is None:
            model_sigma, calib, loss, sensor = s, K, lo, body_P_sensor
        elif s != model_sigma or lo != loss or not K.equals(calib):
            raise NotImplementedError("all stereo factors of one graph must share one noise model and one Cal3_S2Stereo")
        elif not _same_sensor(body_P_sensor, sensor):
            raise NotImplementedError("all stereo factors of one graph must share one body_P_sensor (or all have none)")

    def check_mono_model(model, K, body_P_sensor):
        if model.dim() != 2 or not model.is_isotropic():
            raise NotImplementedError("monocular projection factors need an isotropic 2-dimensional noise model "
                                      "(Isotropic.Sigma(2, sigma)), optionally wrapped in noiseModel.Robust")
        s = float(model.sigmas()[0])
        rob = model.robust() if isinstance(model, _Robust) else None
        lo = (rob.kind, rob.k) if rob is not None else None
        if mono["sigma"] is None:
            mono.update(sigma=s, calib=K, loss=lo, sensor=body_P_sensor)
        elif s != mono["sigma"] or lo != mono["loss"] or not K.equals(mono["calib"]):
            raise NotImplementedError("all monocular projection factors of one graph must share one noise model and one Cal3_S2")
        elif not _same_sensor(body_P_sensor, mono["sensor"]):
            raise NotImplementedError("all monocular projection factors of one graph must share one body_P_sensor (or all "
                                      "have none)")

    def add_mono(m2, pk, lk):
        """(u, v) rows -> (u, unused, v) rows of the one observation list"""
        m2 = np.asarray(m2, dtype=float).reshape(-1, 2)
        m3 = np.zeros((len(m2), 3))
        m3[:, 0], m3[:, 2] = m2[:, 0], m2[:, 1]
        meas.append(m3); pkeys.append(np.asarray(pk, dtype=np.int64)); lkeys.append(np.asarray(lk, dtype=np.int64))
        mono_n.append(len(m3))

    mono_single = ([], [], [])
    # single GenericStereoFactor3D objects were recorded column-wise when they were added (NonlinearFactorGraph._record):
    # only the O(#keyframes) other factors are visited here
    for f in graph._other:
        if isinstance(f, StereoFactorBlock):
            check_model(f._model, f._K, f._sensor)
            meas.append(f.meas); pkeys.append(f.pose_keys); lkeys.append(f.landmark_keys); mono_n.append(0)
        elif isinstance(f, ProjectionFactorBlock):
            check_mono_model(f._model, f._K, f._sensor)
            add_mono(f.meas, f.pose_keys, f.landmark_keys)
        elif isinstance(f, GenericProjectionFactorCal3_S2):       # a subclass instance: not recorded column-wise
            check_mono_model(f._model, f._K, f._sensor)
            mono_single[0].append(f._measured); mono_single[1].append(f._keys[0]); mono_single[2].append(f._keys[1])
        elif isinstance(f, GenericStereoFactor3D):       # a subclass instance: not recorded column-wise
            check_model(f._model, f._K, f._sensor)
            single_m.append(f._measured._m); single_p.append(f._keys[0]); single_l.append(f._keys[1])
        elif isinstance(f, PriorFactorPose3):
            prior_pose.append(f)
        elif isinstance(f, BetweenFactorPose3):
            between_f.append(f)
        elif isinstance(f, _PoseMeasFactor):
            pose_meas_f.append(f)
        elif isinstance(f, LinearContainerFactor):
            if container is not None:
                raise NotImplementedError("more than one LinearContainerFactor in a graph is not supported")
            container = f
        elif isinstance(f, PriorFactorVector):
            prior_vec.append(f)
        elif isinstance(f, ImuFactor):
            imu_f.append(f)
        elif isinstance(f, CombinedImuFactor):
            cimu_f.append(f)
        elif isinstance(f, DvlVelocityFactor):
            dvl_f.append(f)
        elif isinstance(f, (PriorFactorConstantBias, BetweenFactorConstantBias)):
            bias_f.append(f)
        elif isinstance(f, CustomFactor):
            low = lower_reference_dvl_factor(f)
            if low is not None:
                if not dvl_f:
                    import warnings
                    warnings.warn("gtsam.CustomFactor(V(i), X(i), partial(velocity_error, m)) of batch.py:241-250 is solved as "
                                  "DvlVelocityFactor: same residual R_i m - v_i, analytic Jacobians instead of the "
                                  "callback's ill-formed ones (SURVEY.md D7)", stacklevel=3)
                dvl_f.append(low)
                continue
            raise NotImplementedError(
                "gtsam.CustomFactor (a Python callback per factor) cannot run on the GPU; the reference's DVL factor "
                "(batch.py:241-250) additionally returns ill-formed Jacobians (SURVEY.md D7): use "
                "gtsam.DvlVelocityFactor(noise, V(i), X(i), measurement) instead")
        else:
            raise NotImplementedError(f"factor type {type(f).__name__} is not supported by the MI355X optimizer")
    c_meas, c_pk, c_lk, c_model, c_K, c_mixed = graph._stereo_columns()
    if len(c_pk):
        if c_mixed:
            raise NotImplementedError("all stereo factors of one graph must share one noise model, one Cal3_S2Stereo and one "
                                      "body_P_sensor (or have none)")
        check_model(c_model, c_K, graph._st_sensor)
        meas.append(c_meas); pkeys.append(c_pk); lkeys.append(c_lk); mono_n.append(0)
    if single_m:
        meas.append(np.asarray(single_m, dtype=float).reshape(-1, 3))
        pkeys.append(np.asarray(single_p, dtype=np.int64)); lkeys.append(np.asarray(single_l, dtype=np.int64)); mono_n.append(0)
    m_meas, m_pk, m_lk, m_model, m_K, m_mixed = graph._mono_columns()
    if len(m_pk):
        if m_mixed:
            raise NotImplementedError("all monocular projection factors of one graph must share one noise model, one Cal3_S2 "
                                      "and one body_P_sensor (or have none)")
        check_mono_model(m_model, m_K, graph._mo_sensor)
        add_mono(m_meas, m_pk, m_lk)
    if mono_single[0]:
        add_mono(*mono_single)
    has_mono = mono["sigma"] is not None
    if has_mono and model_sigma is not None:
        # one graph, one extrinsic and one mEstimator: the kernels take a single vus_ba_sensor and a single vus_ba_loss
        if not _same_sensor(mono["sensor"], sensor):
            raise NotImplementedError("the monocular projection factors and the stereo factors of one graph must share one "
                                      "body_P_sensor (or all have none)")
        if mono["loss"] != loss:
            raise NotImplementedError("the monocular projection factors and the stereo factors of one graph must share one "
                                      "robust mEstimator and parameter (or all be Gaussian); their sigmas may differ")
    elif has_mono:                  # a graph of mono factors only: their extrinsic and loss are the graph's
        loss, sensor = mono["loss"], mono["sensor"]
    mono_flags = np.concatenate([np.full(len(m), bool(k)) for m, k in zip(meas, mono_n)]) if has_mono else None
    cat = lambda parts, empty: parts[0] if len(parts) == 1 else (np.concatenate(parts) if parts else empty)
    meas = cat(meas, np.zeros((0, 3)))
    pkeys = cat(pkeys, np.zeros(0, np.int64))
    lkeys = cat(lkeys, np.zeros(0, np.int64))

    # variables: vectorised for array-backed Values blocks, per object only for individually inserted ones
    pose_keys, poses = values._pose3_table()
    if len(pose_keys) == 0:
        raise RuntimeError("the Values hold no Pose3 variable")
    if device is not None:
        # key -> index on the GPU by csrc/pack.hip (vus_keys_to_indices: radix sort of the landmark keys + ranks of the
        # distinct ones; vus_lookup_keys: binary search in the pose table), not by torch.unique / searchsorted
        import torch
        from .. import _lib
        dev = torch.device(device)
        n = len(lkeys)
        lk, pk = torch.from_numpy(lkeys).to(dev), torch.from_numpy(pkeys).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        lm_idx, pose_idx = torch.empty(n, **i32), torch.empty(n, **i32)
        uniq = torch.empty(n, dtype=torch.int64, device=dev)
        counters = torch.empty(2, **i32)                       # [n_unique, first_miss]
        nbytes = int(_lib.load().vus_pack_work_bytes(n))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pose_keys_t = torch.from_numpy(pose_keys).to(dev)
        p, st = _lib.ptr, _lib.current_stream_ptr()
        _lib.call("vus_keys_to_indices", p(lk), n, p(lm_idx), p(uniq), p(counters), p(work), nbytes, st)
        _lib.call("vus_lookup_keys", p(pose_keys_t), len(pose_keys), p(pk), n, p(pose_idx), p(counters[1:]), st)
        n_unique, miss = (int(v) for v in counters.tolist())
        if n and miss != 0x7F7F7F7F:
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(int(pkeys[miss]))}\", which does not exist in the Values.")
        lm_keys = uniq[:n_unique].cpu().numpy()
        meas = torch.from_numpy(meas).to(dev)
    else:
        lm_keys, lm_idx = np.unique(lkeys, return_inverse=True)
        upk = np.unique(pkeys)
        at = np.minimum(np.searchsorted(pose_keys, upk), len(pose_keys) - 1)
        if len(upk) and bool((pose_keys[at] != upk).any()):
            k = int(upk[np.nonzero(pose_keys[at] != upk)[0][0]])
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(k)}\", which does not exist in the Values.")
        pose_idx = np.searchsorted(pose_keys, pkeys).astype(np.int32)
        lm_idx = lm_idx.astype(np.int32)
    points = values.point3_block(lm_keys)

    pr_idx, pr_T, pr_s = [], [], []
    for f in prior_pose:
        k = f._keys[0]
        j = int(np.searchsorted(pose_keys, k))
        if j >= len(pose_keys) or pose_keys[j] != k:
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(k)}\", which does not exist in the Values.")
        pr_idx.append(j); pr_T.append(f._prior.flat12()); pr_s.append(f._model.sigmas())
    between = _pack_between(pose_keys, between_f) if between_f else None
    pose_meas = _pack_pose_meas(pose_keys, pose_meas_f) if pose_meas_f else None
    window, nav_window = None, None
    if container is not None and container._is_inertial():      # -> ba.NavWindowPrior
        nav_window = container._nav_window(pose_keys)
    elif container is not None:     # -> ba.WindowPrior: (first pose index, x0 [m, 12], H, gradient, constant)
        window = dict(zip(("first", "x0", "H", "g", "c"), container._window(pose_keys)))
    nav = None
    if imu_f or dvl_f or bias_f or cimu_f or nav_window is not None:
        if window is not None:
            raise NotImplementedError("a LinearContainerFactor over Pose3 keys next to inertial factors (ImuFactor, "
                                      "DvlVelocityFactor, bias factors) is not supported: that dense prior serves the pose-only "
                                      "layout; an inertial window takes one over X(i), V(i), B(i)")
        nav, prior_vec = _pack_nav(values, pose_keys, imu_f, dvl_f, prior_vec, bias_f,
                                   per_keyframe=per_keyframe or nav_window is not None, cimu_f=cimu_f)
    aux = _AuxPriors()
    pp_idx, pp_mean, pp_sig = [], [], []
    for f in prior_vec:
        k = f._keys[0]
        j = int(np.searchsorted(lm_keys, k))
        if j < len(lm_keys) and lm_keys[j] == k:      # lm_keys ascend (unique): a prior on an observed landmark
            if f._prior.size != 3:
                raise RuntimeError(f"a prior factor on the landmark {_sym.key_string(k)} needs a 3-vector, not "
                                   f"{f._prior.size} values")
            pp_idx.append(j); pp_mean.append(f._prior); pp_sig.append(f._model.sigmas())
            continue
        if not values.exists(k):
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(k)}\", which does not exist in the Values.")
        aux.add(k, values.atVector(k), f._prior, f._model.sigmas())
    if len(set(aux.keys)) != len(aux.keys):
        raise NotImplementedError("several prior factors on one vector variable are not supported")
    return dict(meas=meas, pose_idx=pose_idx, lm_idx=lm_idx, pose_keys=pose_keys, lm_keys=lm_keys, poses=poses,
                points=points, sigma=model_sigma if model_sigma is not None else 1.0, loss=loss,
                body_P_sensor=sensor.flat12() if sensor is not None else None,
                K=calib.vector6() if calib is not None else np.array([1.0, 1.0, 0.0, 0.0, 0.0, 1.0]),
                mono=mono_flags, mono_K=mono["calib"].vector() if has_mono else None, mono_sigma=mono["sigma"],
                prior_idx=np.asarray(pr_idx, np.int32), prior_T=np.asarray(pr_T, float).reshape(-1, 12),
                prior_sigmas=np.asarray(pr_s, float).reshape(-1, 6), aux=aux, nav=nav, between=between, pose_meas=pose_meas,
                window_prior=window, nav_window_prior=nav_window,
                point_priors=dict(idx=np.asarray(pp_idx, np.int32), mean=np.asarray(pp_mean, float).reshape(-1, 3),
                                  sigmas=np.asarray(pp_sig, float).reshape(-1, 3)) if pp_idx else None)


def _pack_between(pose_keys, between_f):
    """BetweenFactorPose3 -> (i, j, meas [n, 12], sigmas [n, 6], losses [n], span, sqrt_info): pose indices into the sorted
    Pose3 keys, the measured poses, the sigmas (the roots of the covariance diagonal under a full model), each factor's
    (VUS_LOSS_* kind, k), the widest pose distance, and sqrt_info [n, 6, 6] = every factor's R (diag(1 / sigma) for a
    diagonal one) when at least one factor carries a full-covariance noiseModel.Gaussian, else None."""
    from . import _Robust, _is_full, _sqrt_info_of
    bi, bj, bm, bs, bl = [], [], [], [], []
    for f in between_f:
        idx = []
        for k in f._keys:
            j = int(np.searchsorted(pose_keys, k))
            if j >= len(pose_keys) or pose_keys[j] != k:
                raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(k)}\", which does not exist in the Values.")
            idx.append(j)
        rob = f._model.robust() if isinstance(f._model, _Robust) else None
        bi.append(idx[0]); bj.append(idx[1]); bm.append(f._measured.flat12()); bs.append(f._model.sigmas())
        bl.append((rob.kind, rob.k) if rob is not None else (0, 0.0))
    bi, bj = np.asarray(bi, np.int32), np.asarray(bj, np.int32)
    full = any(_is_full(f._model) for f in between_f)
    return dict(i=bi, j=bj, meas=np.asarray(bm, float).reshape(-1, 12), sigmas=np.asarray(bs, float).reshape(-1, 6),
                losses=bl, span=int(np.abs(bi.astype(np.int64) - bj).max()),
                sqrt_info=np.stack([_sqrt_info_of(f._model) for f in between_f]) if full else None)


def _pack_pose_meas(pose_keys, pose_meas_f):
    """GPSFactor / GPSFactorArm / PoseTranslationPrior3D / PoseRotationPrior3D -> (idx, kind, meas [n, 9], sigmas [n, 3],
    losses [n], keys [n]) in graph order: pose indices into the sorted Pose3 keys, the VUS_POSE_MEAS_* kinds, the rows of
    include/vus_pose_meas.h, the diagonal sigmas, each factor's (VUS_LOSS_* kind, k) and its pose key."""
    from . import _Robust
    idx, kind, meas, sig, losses, keys = [], [], [], [], [], []
    for f in pose_meas_f:
        k = f._keys[0]
        j = int(np.searchsorted(pose_keys, k))
        if j >= len(pose_keys) or pose_keys[j] != k:
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(k)}\", which does not exist in the Values.")
        rob = f._model.robust() if isinstance(f._model, _Robust) else None
        idx.append(j); kind.append(f._kind); meas.append(f._row9()); sig.append(f._model.sigmas()); keys.append(k)
        losses.append((rob.kind, rob.k) if rob is not None else (0, 0.0))
    return dict(idx=np.asarray(idx, np.int32), kind=np.asarray(kind, np.int32), meas=np.asarray(meas, float).reshape(-1, 9),
                sigmas=np.asarray(sig, float).reshape(-1, 3), losses=losses, keys=np.asarray(keys, np.int64))


def _pack_nav(values, pose_keys, imu_f, dvl_f, prior_vec, bias_f=(), per_keyframe=False, cimu_f=()):
    """Velocity / bias side of the graph (batch.py:274-293): every pose X(i) needs a velocity V(i) with the same
    index; either one shared bias key (batch.py:238 passes B(0) to every ImuFactor) or, when the graph has bias factors
    or several bias keys or a CombinedImuFactor (`cimu_f`, packed by _pack_combined) or `per_keyframe` asks for it, one bias
    B(i) per keyframe (_pack_bias_walk)."""
    from . import _ConstantBias
    pidx = {int(k): i for i, k in enumerate(pose_keys.tolist())}
    vel_keys = []
    for k in pose_keys.tolist():
        vk = _sym.symbol("v", _sym.symbolIndex(k))
        if not values.exists(vk):
            raise RuntimeError(f"Attempting to at the key \"{_sym.key_string(vk)}\", which does not exist in the Values.")
        vel_keys.append(vk)
    vidx = {k: i for i, k in enumerate(vel_keys)}
    vels = np.stack([values.atVector(k) for k in vel_keys])
    if vels.shape[1] != 3:
        raise RuntimeError("velocity variables must be 3-vectors")
    bias_keys = sorted({f._keys[4] for f in imu_f})
    per_keyframe = bool(per_keyframe) or bool(bias_f) or len(bias_keys) > 1 or bool(cimu_f)
    if per_keyframe:
        bias_keys, biases, bbetween, bprior = _pack_bias_walk(values, pose_keys, imu_f, bias_f)
    bias_key = bias_keys[0] if bias_keys and not per_keyframe else None
    bias = values.atConstantBias(bias_key).vector() if bias_key is not None else np.zeros(6)
    if per_keyframe:
        bias = biases
    imu_i, imu_j, pims, Ws, grav = [], [], [], [], None
    for f in imu_f:
        ki, kvi, kj, kvj, _ = f._keys
        if ki not in pidx or kj not in pidx or vidx.get(kvi) != pidx[ki] or vidx.get(kvj) != pidx[kj]:
            raise RuntimeError("ImuFactor: its pose / velocity keys are not X(i), V(i), X(j), V(j) of the Values")
        if pidx[kj] != pidx[ki] + 1:
            raise NotImplementedError("ImuFactor between non-consecutive keyframes is not supported")
        if grav is not None and not np.array_equal(grav, f.gravity):
            raise NotImplementedError("all ImuFactors must share one gravity vector")
        grav = f.gravity
        imu_i.append(pidx[ki]); imu_j.append(pidx[kj]); pims.append(f.pim); Ws.append(f.W)
    combined = None
    if cimu_f:
        combined, grav = _pack_combined(cimu_f, pidx, vidx, bias_keys, grav)
    dvl_p, dvl_m, dvl_s = [], [], []
    for f in dvl_f:
        kv, kx = f._keys
        if kx not in pidx or vidx.get(kv) != pidx[kx]:
            raise RuntimeError("DvlVelocityFactor: its keys are not (V(i), X(i)) of the Values")
        dvl_p.append(pidx[kx]); dvl_m.append(f.measured); dvl_s.append(float(f._model.sigmas()[0]))
    vp_i, vp_v, vp_s, rest = [], [], [], []
    for f in prior_vec:
        k = f._keys[0]
        if k in vidx:
            vp_i.append(vidx[k]); vp_v.append(f._prior); vp_s.append(f._model.sigmas())
        else:
            rest.append(f)
    nav = dict(vel_keys=vel_keys, bias_key=bias_key, vels=vels, bias=bias, per_keyframe=per_keyframe,
               bias_keys=bias_keys if per_keyframe else None, bbetween=bbetween if per_keyframe else None,
               bprior=bprior if per_keyframe else None, combined=combined,
               gravity=grav if grav is not None else np.array([0.0, 0.0, -9.81]),
               imu=(np.asarray(imu_i, np.int32), np.asarray(imu_j, np.int32), np.asarray(pims, float).reshape(-1, 148),
                    np.asarray(Ws, float).reshape(-1, 81)) if imu_f else None,
               dvl=(np.asarray(dvl_p, np.int32), np.asarray(dvl_m, float).reshape(-1, 3), np.asarray(dvl_s, float)) if dvl_f else None,
               vprior=(np.asarray(vp_i, np.int32), np.asarray(vp_v, float).reshape(-1, 3),
                       np.asarray(vp_s, float).reshape(-1, 3)) if vp_i else None)
    return nav, rest


def _pack_combined(cimu_f, pidx, vidx, bias_keys, grav):
    """CombinedImuFactor -> (i [n], pim [n, 148], W [n, 225]) for ba.CombinedImuFactors and the graph's gravity: every
    factor on X(i), V(i), X(i+1), V(i+1), B(i), B(i+1) of consecutive keyframes.  Anything else is refused with the reason."""
    name = _sym.key_string
    ci, pims, Ws = [], [], []
    for f in cimu_f:
        ki, kvi, kj, kvj, kbi, kbj = f._keys
        what = f"CombinedImuFactor({name(ki)}, {name(kvi)}, {name(kj)}, {name(kvj)}, {name(kbi)}, {name(kbj)})"
        if ki not in pidx or kj not in pidx or vidx.get(kvi) != pidx[ki] or vidx.get(kvj) != pidx[kj]:
            raise RuntimeError(f"{what}: its pose / velocity keys are not X(i), V(i), X(j), V(j) of the Values")
        i, j = pidx[ki], pidx[kj]
        if j != i + 1:
            raise NotImplementedError(f"{what}: a CombinedImuFactor between non-consecutive keyframes is not supported (the "
                                      "band holds the couplings of neighbouring keyframes only)")
        if kbi != bias_keys[i] or kbj != bias_keys[j]:
            raise NotImplementedError(f"{what}: its biases must be {name(bias_keys[i])} and {name(bias_keys[j])}, the biases of "
                                      "its two keyframes")
        if grav is not None and not np.array_equal(grav, f.gravity):
            raise NotImplementedError("all ImuFactors and CombinedImuFactors must share one gravity vector")
        grav = f.gravity
        ci.append(i); pims.append(f.pim); Ws.append(f.W)
    return (np.asarray(ci, np.int32), np.asarray(pims, float).reshape(-1, 148), np.asarray(Ws, float).reshape(-1, 225)), grav


def _pack_bias_walk(values, pose_keys, imu_f, bias_f):
    """One bias per keyframe (GTSAM's ImuFactorsExample): B(i) for every X(i), ImuFactor(X(i), V(i), X(i+1), V(i+1), B(i)),
    BetweenFactorConstantBias only between consecutive biases, PriorFactorConstantBias with a diagonal or isotropic
    model.  Returns (bias keys, biases [n, 6], bbetween = (i, j, meas, sigmas) or None, bprior = (idx, mean, sigmas) or
    None).  Anything else is refused with the reason."""
    from . import PriorFactorConstantBias, _Robust
    n = len(pose_keys)
    pidx = {int(k): i for i, k in enumerate(pose_keys.tolist())}
    bias_keys = [_sym.symbol("b", _sym.symbolIndex(int(k))) for k in pose_keys.tolist()]
    bidx = {k: i for i, k in enumerate(bias_keys)}
    name = _sym.key_string
    per_key = {}
    for f in imu_f:
        per_key.setdefault(f._keys[4], []).append(f)
    shared = [k for k, fs in per_key.items() if len(fs) > 1]
    if shared:
        raise NotImplementedError(
            f"the graph mixes one shared bias ({name(shared[0])} in {len(per_key[shared[0]])} ImuFactors) with per-keyframe "
            "biases (bias factors or several bias keys): give each ImuFactor the bias B(i) of its earlier keyframe")
    for k in bias_keys:
        if not values.exists(k):
            raise RuntimeError(f"per-keyframe biases: the bias {name(k)} of keyframe {name(pose_keys[bidx[k]])} is missing "
                               f"(Attempting to at the key \"{name(k)}\", which does not exist in the Values.)")
    for f in imu_f:
        i = pidx.get(f._keys[0])
        if i is not None and f._keys[4] != bias_keys[i]:
            raise NotImplementedError(f"ImuFactor({name(f._keys[0])}, .., {name(f._keys[2])}) uses the bias "
                                      f"{name(f._keys[4])}; with per-keyframe biases it must use {name(bias_keys[i])}, the "
                                      "bias of its earlier keyframe")
    bb_i, bb_m, bb_s, bp_i, bp_m, bp_s = [], [], [], [], [], []
    for f in bias_f:
        what = type(f).__name__
        if isinstance(f._model, _Robust):
            raise NotImplementedError(f"{what} on {', '.join(name(k) for k in f._keys)}: robust noise models on bias factors "
                                      "are not supported")
        if f._model.dim() != 6:
            raise RuntimeError(f"{what}: needs a 6-dimensional noise model")
        for k in f._keys:
            if k not in bidx:
                raise NotImplementedError(f"{what} on {name(k)}: not the bias B(i) of a keyframe X(i)")
        if isinstance(f, PriorFactorConstantBias):
            bp_i.append(bidx[f._keys[0]]); bp_m.append(f._prior.vector()); bp_s.append(f._model.sigmas())
        else:
            a, b = bidx[f._keys[0]], bidx[f._keys[1]]
            if b != a + 1:
                raise NotImplementedError(f"BetweenFactorConstantBias({name(f._keys[0])}, {name(f._keys[1])}): only "
                                          "consecutive biases B(i), B(i+1) can be joined")
            bb_i.append(a); bb_m.append(f._measured.vector()); bb_s.append(f._model.sigmas())
    biases = np.stack([values.atConstantBias(k).vector() for k in bias_keys])
    bbetween = (np.asarray(bb_i, np.int32), np.asarray(bb_i, np.int32) + 1, np.asarray(bb_m, float).reshape(-1, 6),
                np.asarray(bb_s, float).reshape(-1, 6)) if bb_i else None
    bprior = (np.asarray(bp_i, np.int32), np.asarray(bp_m, float).reshape(-1, 6),
              np.asarray(bp_s, float).reshape(-1, 6)) if bp_i else None
    assert len(biases) == n
    return bias_keys, biases, bbetween, bprior


def _build_solver(pg, device="cuda:0", long_span=None, min_span=0):
    """long_span: LevenbergMarquardtParams.longClosureSpan -- between factors spanning more poses form the long set, and
    the band follows the rest.  min_span: the band is at least this many poses wide (a fixed-lag smoother's sub-problem,
    whose marginal must fit the band); a LinearContainerFactor's width feeds the band in the same way."""
    from ..ba import (StereoBAProblem, StereoBASolver, NavBASolver, NavFactors, NavBiasBASolver, NavBiasFactors,
                      BetweenFactors, PointPriors, PoseMeasurements, WindowPrior, NavWindowPrior, CombinedImuFactors)
    nav = pg.get("nav")
    btw = pg.get("between")
    walk = bool(nav) and nav.get("per_keyframe", False)
    stride = (3 if walk else 2) if nav else 1
    n_poses = len(pg["pose_keys"])
    between_span = btw["span"] if btw else 0
    if btw and long_span is not None:
        spans = np.abs(btw["i"].astype(np.int64) - btw["j"])
        between_span = int(spans[spans <= long_span].max(initial=0))
    win, nwin = pg.get("window_prior"), pg.get("nav_window_prior")
    if (win is not None or nwin is not None) and btw and long_span is not None:
        raise NotImplementedError("a LinearContainerFactor together with long closures (setLongClosureSpan) is not supported")
    # an inertial prior over m keyframes needs 3 m - 1 nodes (B of the last against X of the first): m poses' worth
    between_span = max(between_span, int(min_span), len(win["x0"]) - 1 if win is not None else 0,
                       len(nwin["x0"]) if nwin is not None else 0)
    cimu = nav.get("combined") if nav else None
    extra = dict(combined_imu=True) if cimu is not None else {}         # without one the problem is built as before
    prob =StereoBAProblem(pg["pose_idx"], pg["lm_idx"], pg["meas"], n_poses, len(pg["lm_keys"]),
                           pg["K"], pg["sigma"], prior_pose=pg["prior_idx"], prior_T=pg["prior_T"],
                           prior_sigmas=pg["prior_sigmas"], device=device, pose_stride=stride,
                           loss=pg.get("loss"), between_span=between_span,
                           body_P_sensor=pg.get("body_P_sensor"), mono=pg.get("mono"), mono_K=pg.get("mono_K"),
                           mono_sigma=pg.get("mono_sigma"), **extra)
    # a factor the landmark band already covers stays in the band whatever long_span says
    max_span = None if long_span is None else max(int(long_span), prob.band // stride)
    bf = BetweenFactors(btw["i"], btw["j"], btw["meas"], btw["sigmas"], n_poses, pose_stride=stride,
                        loss=list(btw["losses"]), device=device, max_span=max_span,
                        sqrt_info=btw.get("sqrt_info")) if btw else None
    pp = pg.get("point_priors")
    pf = PointPriors(pp["idx"], pp["mean"], pp["sigmas"], len(pg["lm_keys"]), device=device) if pp else None
    pm = pg.get("pose_meas")
    mf = PoseMeasurements(pm["idx"], pm["kind"], pm["meas"], pm["sigmas"], n_poses, pose_stride=stride,
                          loss=list(pm["losses"]), device=device) if pm else None
    if walk:
        nf = NavBiasFactors(nav["gravity"], imu=nav["imu"], dvl=nav["dvl"], vprior=nav["vprior"], bbetween=nav["bbetween"],
                            bprior=nav["bprior"], device=device)
        nw = NavWindowPrior(nwin["first"], nwin["x0"], nwin["v0"], nwin["b0"], nwin["H"], nwin["g"], nwin["c"], n_poses,
                            device=device) if nwin is not None else None
        if cimu is None:
            return prob, NavBiasBASolver(prob, nf, bf, pf, mf, window_prior=nw)
        cf = CombinedImuFactors(nav["gravity"], cimu[0], cimu[1], cimu[2], device=device)
        return prob, NavBiasBASolver(prob, nf, bf, pf, mf, window_prior=nw, combined=cf)
    if nav:
        nf = NavFactors(nav["gravity"], imu=nav["imu"], dvl=nav["dvl"], vprior=nav["vprior"], device=device)
        return prob, NavBASolver(prob, nf, bf, pf, mf)
    wf = WindowPrior(win["first"], win["x0"], win["H"], win["g"], win["c"], n_poses, device=device) if win is not None else None
    return prob, StereoBASolver(prob, bf, pf, pose_meas=mf, window_prior=wf)


def graph_error(graph, values) -> float:
    import torch
    import torch as _torch
    pg = _pack_graph(graph, values, "cuda:0" if _torch.cuda.is_available() else None)
    prob, sv = _build_solver(pg)
    dev = prob.device
    poses = torch.from_numpy(pg["poses"]).to(dev)
    points = torch.from_numpy(pg["points"]).to(dev)
    e = (sv.error(poses, points) + sv.between_error(poses) + sv.closure_error(poses) + sv.point_prior_error(points) +
         sv.pose_meas_error(poses))
    if pg.get("window_prior") is not None:
        e += sv.window_prior_error(poses)
    if pg.get("nav"):
        vels, bias = torch.from_numpy(pg["nav"]["vels"]).to(dev), torch.from_numpy(pg["nav"]["bias"]).to(dev)
        e += sv.nav_error(poses, vels, bias)
        if pg["nav"].get("combined") is not None:
            e += sv.cimu_error(poses, vels, bias)
        if pg.get("nav_window_prior") is not None:
            e += sv.nav_window_prior_error(poses, vels, bias)
    return e + pg["aux"].error()


class LevenbergMarquardtOptimizer:
    """gtsam.LevenbergMarquardtOptimizer(graph, initialValues, params=LevenbergMarquardtParams())."""

    def __init__(self, graph, initialValues, params: Optional[LevenbergMarquardtParams] = None, device="cuda:0",
                 per_keyframe_bias=False):
        """EXTENSION `per_keyframe_bias`: solve the inertial side with one bias B(i) per keyframe even where the graph alone
        would be read as the shared-bias layout (a single ImuFactor and no bias factor): a fixed-lag window of two keyframes."""
        self._graph, self._initial = graph, initialValues
        self._per_keyframe = bool(per_keyframe_bias)
        self._params = params or LevenbergMarquardtParams()
        self._device = device
        self._result = None
        self._report = None

    def optimize(self):
        """Runs LM to convergence and returns a NEW Values; the inputs are left untouched."""
        import torch
        from . import Values, Pose3, _ConstantBias
        from .. import _lib
        _lib.require_gpu()                      # no CPU fallback: fail before any work is done
        import os
        import time
        prof = os.environ.get("VUS_PROFILE_BOUNDARY") == "1"     # phase times (synchronising): bench.py's drop-in breakdown
        marks = [("start", time.perf_counter())]

        def mark(name):
            if prof:
                torch.cuda.synchronize()
                marks.append((name, time.perf_counter()))
        pg = _pack_graph(self._graph, self._initial, self._device, self._per_keyframe)
        mark("pack_graph_host+upload")
        prob, sv = _build_solver(pg, self._device, self._params.longClosureSpan)
        mark("structure+workspace")
        aux = pg["aux"] if pg["aux"].keys else None
        nav = pg.get("nav")
        dev = prob.device
        if nav:
            if aux is not None:
                raise NotImplementedError("prior factors on extra vector variables next to inertial factors are not supported")
            poses, vels, bias, points, rep = sv.optimize(torch.from_numpy(pg["poses"]).to(dev), torch.from_numpy(nav["vels"]).to(dev),
                                                         torch.from_numpy(nav["bias"]).to(dev),
                                                         torch.from_numpy(pg["points"]).to(dev), self._params._to_lm())
            vels, bias = vels.cpu().numpy(), bias.cpu().numpy()
        else:
            poses, points, rep = sv.optimize(torch.from_numpy(pg["poses"]).to(dev), torch.from_numpy(pg["points"]).to(dev),
                                             self._params._to_lm(), aux=aux)
        mark("lm")
        rep.stereo_weights = None
        if prob.robust:           # final IRLS weights per stereo factor, identified by its (pose key, landmark key)
            w = sv.stereo_weights(poses, points).cpu().numpy()
            pi, li = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x, dtype=np.int64) for x in (pg["pose_idx"], pg["lm_idx"]))
            rep.stereo_weights = (pg["pose_keys"][pi], np.asarray(pg["lm_keys"])[li], w)
        rep.pose_meas_weights = None
        if sv.M is not None and sv.M.robust:     # final IRLS weights per position / attitude fix, graph order, by pose key
            rep.pose_meas_weights = (pg["pose_meas"]["keys"], sv.pose_meas_weights(poses).cpu().numpy())
        poses, points = poses.cpu().numpy(), points.cpu().numpy()
        out = Values(self._initial)
        if nav:
            for k, v in zip(nav["vel_keys"], vels):
                out.update(k, v)
            if nav["bias_key"] is not None:
                out.update(nav["bias_key"], _ConstantBias(bias[:3], bias[3:]))
            for k, b in zip(nav["bias_keys"] or (), bias.reshape(-1, 6) if nav["per_keyframe"] else ()):
                out.update(k, _ConstantBias(b[:3], b[3:]))
        out._store_rows("pose3", pg["pose_keys"], poses)
        out._store_rows("point3", pg["lm_keys"], points)
        if aux is not None:
            for k, x in zip(aux.keys, aux.x):
                out.update(k, x)
        mark("read_back")
        if prof:
            rep.boundary_ms = {n: round(1e3 * (t - marks[i][1]), 3) for i, (n, t) in enumerate(marks[1:])}
        self._result, self._report = out, rep
        return out

    def optimizeSafely(self):
        return self.optimize()

    def values(self):
        return self._result if self._result is not None else self._initial

    def error(self):
        if self._report is not None:
            return self._report.final_error
        return graph_error(self._graph, self._initial)

    def iterations(self):
        return 0 if self._report is None else self._report.iterations

    def lambda_(self):
        return self._params.lambdaInitial if self._report is None else self._report.final_lambda

    def report(self):
        """EXTENSION: the LMReport of the last optimize() (error / lambda history, timings).  With robust stereo factors
        its `stereo_weights` = (pose keys, landmark keys, w) holds every stereo factor's final weight w(d); else None.  With
        a noiseModel.Robust on any GPSFactor / GPSFactorArm / PoseTranslationPrior3D / PoseRotationPrior3D its
        `pose_meas_weights` = (pose keys, w) holds the final weight of every such factor, in graph order; else None."""
        return self._report
