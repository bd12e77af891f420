"""gtsam_unstable-shaped module: BatchFixedLagSmoother on the MI355X.

A fixed-lag smoother keeps the keyframes of the last `smootherLag` seconds and turns everything older into ONE Gaussian
prior on the keyframes that remain (a gtsam.LinearContainerFactor holding a gtsam.HessianFactor, solved as the dense
window prior of include/vus_fixed_lag.h).  Every update() optimises the window with the existing
LevenbergMarquardtOptimizer and then marginalises the expired keyframes with StereoBASolver.marginalize_head.

DEVIATION from upstream (the rule OKVIS-style windows use): a landmark seen from an expired keyframe is marginalised
only if its OWN timestamp has expired; if it is still alive, its factors from the expired keyframes are DISCARDED instead
of absorbed, and the count is reported.  Absorbing them would tie the prior to a landmark, and landmarks would stop being
independent given the poses -- the independence the whole Schur path of the solver rests on.

Served: stereo and monocular projection factors (single or in blocks), PriorFactorPose3, BetweenFactorPose3, the position /
attitude fixes, PriorFactorPoint3 -- and, in the per-keyframe-bias layout, ImuFactor, DvlVelocityFactor,
PriorFactorConstantBias, BetweenFactorConstantBias and PriorFactorVector on a velocity.  Every keyframe of such a window
carries X(i), V(i) and B(i), all three with the timestamp of X(i); the prior then covers all three (ba.NavWindowPrior) and
all three leave together.  An inertial factor in any other layout -- a keyframe without one of its three keys, one shared
bias -- is refused by name, and so is gtsam.CustomFactor.
"""
from typing import Dict

import numpy as np

from .. import gtsam as _g
from ..gtsam import symbol_shorthand as _sym
from ..gtsam.optimizer import LevenbergMarquardtParams, LevenbergMarquardtOptimizer, _pack_graph, _build_solver

_BLOCKS = (_g.StereoFactorBlock, _g.ProjectionFactorBlock)
_SINGLE_PROJ = (_g.GenericStereoFactor3D, _g.GenericProjectionFactorCal3_S2)
_POSE_SIDE = (_g.PriorFactorPose3, _g.BetweenFactorPose3, _g._PoseMeasFactor, _g.LinearContainerFactor)
_SERVED_INERTIAL = (_g.ImuFactor, _g.DvlVelocityFactor, _g.PriorFactorConstantBias, _g.BetweenFactorConstantBias)


class FixedLagSmootherKeyTimestampMap(dict):
    """gtsam_unstable.FixedLagSmootherKeyTimestampMap: key -> timestamp; insert((key, t)) as upstream."""

    def insert(self, pair):
        k, t = pair
        self[int(k)] = float(t)


def _missing(key):
    return RuntimeError(f"Attempting to at the key \"{_sym.key_string(int(key))}\", which does not exist in the Values.")


def _is_velocity_prior(f):
    return type(f) is _g.PriorFactorVector and _sym.symbolChr(f._keys[0]) == "v"


def _on_keyframe_side(f):
    """A factor on keyframe variables only (poses, velocities, biases): absorbed as soon as one of its keys expires."""
    return isinstance(f, _POSE_SIDE + _SERVED_INERTIAL) or _is_velocity_prior(f)


def _inertial_window(factors):
    """Whether the factors make an inertial window: one in which every keyframe carries X(i), V(i) and B(i)."""
    return any(isinstance(f, _SERVED_INERTIAL) or _is_velocity_prior(f)
               or (isinstance(f, _g.LinearContainerFactor) and f._is_inertial()) for f in factors)


def keyframe_keys(pose_key):
    """X(i), V(i), B(i) of the keyframe whose pose key is X(i)."""
    i = _sym.symbolIndex(int(pose_key))
    return [_sym.symbol(c, i) for c in "xvb"]


def _pose_key_of(key):
    """The pose key X(i) of a keyframe variable X(i), V(i) or B(i); any other key unchanged."""
    return _sym.symbol("x", _sym.symbolIndex(int(key))) if _sym.symbolChr(int(key)) in "vb" else int(key)


def absorbed_set(pose_factors, projections, point_priors, expired_poses, timestamps, cut):
    """The rule that makes a sliding window usable, on keys alone.
      pose_factors  [keys of a pose-side factor]          (priors, between factors, fixes, the previous container; in an
                                                           inertial window the inertial-side factors too, and
                                                           `expired_poses` then holds X(i), V(i) AND B(i) of every expired
                                                           keyframe: a factor touching any of them is absorbed)
      projections   [(pose key, landmark key)]             one per projection factor (a row of a block counts as one)
      point_priors  [landmark key]
    Returns (absorb_pose [bool], absorb_proj [bool], discard_proj [bool], absorb_pp [bool], marginalised landmark keys):
      - every pose-side factor touching an expired pose is absorbed;
      - a landmark seen from an expired pose whose own timestamp is older than `cut` is marginalised: all its projection
        factors, those from kept poses too, and its point priors are absorbed;
      - a landmark seen from an expired pose that is still alive is kept: its factors from the expired poses are discarded;
      - an expired landmark no expired pose sees stays until one does."""
    expired = set(int(k) for k in expired_poses)
    absorb_pose = [any(int(k) in expired for k in keys) for keys in pose_factors]
    seen = {int(l) for p, l in projections if int(p) in expired}
    gone = {l for l in seen if timestamps[l] < cut}
    absorb_proj = [int(l) in gone for _, l in projections]
    discard_proj = [int(p) in expired and int(l) not in gone for p, l in projections]
    absorb_pp = [int(l) in gone for l in point_priors]
    return absorb_pose, absorb_proj, discard_proj, absorb_pp, sorted(gone)


class BatchFixedLagSmoother:
    """gtsam_unstable.BatchFixedLagSmoother(smootherLag, params=LevenbergMarquardtParams())."""

    def __init__(self, smootherLag, params=None, device="cuda:0"):
        self._lag = float(smootherLag)
        self._params = params or LevenbergMarquardtParams()
        self._device = device
        self._factors = []                          # factor objects; blocks are re-cut when rows leave
        self._theta = _g.Values()
        self._ts: Dict[int, float] = {}
        self.last_update = dict(marginalized_landmarks=0, discarded_factors=0, absorbed_factors=0, expired_poses=0,
                                seconds=dict(pack=0.0, optimize=0.0, marginalize=0.0))

    # -- upstream's accessors -----------------------------------------------------------------------------------------
    def smootherLag(self):
        return self._lag

    def params(self):
        return self._params

    def timestamps(self):
        return FixedLagSmootherKeyTimestampMap(self._ts)

    def calculateEstimate(self):
        return _g.Values(self._theta)

    def calculateEstimatePose3(self, key):
        return self._theta.atPose3(key)

    def getLinearizationPoint(self):
        return _g.Values(self._theta)

    def getFactors(self):
        g = _g.NonlinearFactorGraph()
        for f in self._factors:
            g.push_back(f)
        return g

    # -- update -------------------------------------------------------------------------------------------------------
    def update(self, newFactors=None, newTheta=None, timestamps=None):
        import time
        t0 = time.perf_counter()
        new = list(newFactors._factors) if newFactors is not None else []
        for f in new:
            if isinstance(f, _g.CombinedImuFactor):
                raise NotImplementedError("BatchFixedLagSmoother: CombinedImuFactor is not supported -- marginalising keyframes "
                                          "out of a graph that holds one is not implemented; use ImuFactor and "
                                          "BetweenFactorConstantBias in the smoother")
            if isinstance(f, _g.CustomFactor):
                raise NotImplementedError(f"BatchFixedLagSmoother: {type(f).__name__} is not supported -- of the inertial "
                                          "factors the smoother takes ImuFactor, DvlVelocityFactor and the bias factors")
            if not isinstance(f, _BLOCKS + _SINGLE_PROJ + _POSE_SIDE + _SERVED_INERTIAL + (_g.PriorFactorVector,)):
                raise NotImplementedError(f"BatchFixedLagSmoother: factor type {type(f).__name__} is not supported")
        theta, ts = _g.Values(self._theta), dict(self._ts)
        if newTheta is not None:
            for k in newTheta.keys():
                theta.insert(k, newTheta._at(k, object, "at"))
        for f in new:                               # the layout of an inertial factor, before anything else about its keys
            self._refuse_layout(f, theta)
        for k, t in (timestamps or {}).items():     # a timestamp for an existing key replaces it, as upstream
            ts[int(k)] = float(t)
        for f in new:                               # a factor on a removed (or never given) key: upstream's message
            for k in f.keys():
                if not theta.exists(k):
                    raise _missing(k)
        for k in theta.keys():
            if k not in ts:
                raise ValueError(f"BatchFixedLagSmoother: no timestamp for the key {_sym.key_string(k)}")
        factors = self._factors + new
        inertial = _inertial_window(factors)
        if inertial:
            self._check_keyframes(theta, ts)
        graph = _g.NonlinearFactorGraph()
        for f in factors:
            graph.push_back(f)
        t1 = time.perf_counter()
        opt = LevenbergMarquardtOptimizer(graph, theta, self._params, device=self._device, per_keyframe_bias=inertial)
        theta = opt.optimize()
        self.last_report = opt.report()
        t2 = time.perf_counter()
        stats = self._marginalize(factors, theta, ts)
        t3 = time.perf_counter()
        stats["seconds"] = dict(pack=t1 - t0, optimize=t2 - t1, marginalize=t3 - t2)
        self.last_update = stats
        return stats

    @staticmethod
    def _refuse_layout(f, theta):
        """An inertial factor is served in the per-keyframe-bias layout only: every keyframe it touches has X(i), V(i) and
        B(i) in the Values, and an ImuFactor uses the bias of its earlier keyframe."""
        if not (isinstance(f, _SERVED_INERTIAL) or _is_velocity_prior(f)):
            return
        name, what = _sym.key_string, type(f).__name__
        for i in sorted({_sym.symbolIndex(int(k)) for k in f._keys}):
            missing = [k for k in keyframe_keys(_sym.symbol("x", i)) if not theta.exists(k)]
            if missing:
                raise NotImplementedError(
                    f"BatchFixedLagSmoother: {what} on {', '.join(name(int(k)) for k in f._keys)} is not supported in this layout "
                    f"-- an inertial window carries X(i), V(i) and B(i) of every keyframe, and {', '.join(map(name, missing))} "
                    "is not in the Values")
        if isinstance(f, _g.ImuFactor) and _sym.symbolIndex(int(f._keys[4])) != _sym.symbolIndex(int(f._keys[0])):
            raise NotImplementedError(
                f"BatchFixedLagSmoother: ImuFactor({name(int(f._keys[0]))}, .., {name(int(f._keys[2]))}) uses the bias "
                f"{name(int(f._keys[4]))} -- the shared-bias layout is not served by the fixed-lag smoother; of the inertial "
                f"layouts it takes one bias per keyframe, here {name(_sym.symbol('b', _sym.symbolIndex(int(f._keys[0]))))}")

    @staticmethod
    def _check_keyframes(theta, ts):
        """An inertial window: V(i) and B(i) of every keyframe carry the timestamp of X(i), so that all three expire together."""
        pose_keys, _ = theta._pose3_table()
        for pk in pose_keys.tolist():
            kx, kv, kb = keyframe_keys(pk)
            for k in (kv, kb):
                if theta.exists(k) and k in ts and kx in ts and ts[k] != ts[kx]:
                    raise ValueError(f"BatchFixedLagSmoother: the key {_sym.key_string(k)} has the timestamp {ts[k]}, its keyframe "
                                     f"{_sym.key_string(kx)} has {ts[kx]}: X(i), V(i) and B(i) share one timestamp")

    def _marginalize(self, factors, theta, ts):
        """Steps 2-4 of update(): expired poses, the absorbed set, the new prior; commits the window."""
        inertial = _inertial_window(factors)
        stats = dict(marginalized_landmarks=0, discarded_factors=0, absorbed_factors=0, expired_poses=0)
        pose_keys, _ = theta._pose3_table()
        cut = max(ts.values()) - self._lag
        is_old = np.array([ts[int(k)] < cut for k in pose_keys])
        n_exp = int(is_old.sum())
        if n_exp and not is_old[:n_exp].all():
            raise RuntimeError("BatchFixedLagSmoother: the expired poses are not the leading keys of the sorted pose table")
        if n_exp == len(pose_keys):
            raise RuntimeError("BatchFixedLagSmoother: every pose has expired")
        if n_exp == 0:
            self._factors, self._theta, self._ts = factors, theta, ts
            return stats
        expired = [int(k) for k in pose_keys[:n_exp]]
        # an inertial window: the velocity and the bias of an expired keyframe expire with its pose
        expired_keys = [k for p in expired for k in keyframe_keys(p)] if inertial else expired
        # the factors as key records
        pose_f, proj, proj_at, pps = [], [], [], []
        for i, f in enumerate(factors):
            if isinstance(f, _BLOCKS):
                proj += list(zip(f.pose_keys.tolist(), f.landmark_keys.tolist()))
                proj_at += [(i, r) for r in range(len(f))]
            elif isinstance(f, _SINGLE_PROJ):
                proj.append((f._keys[0], f._keys[1]))
                proj_at.append((i, -1))
            elif _on_keyframe_side(f):
                pose_f.append(i)
            else:
                pps.append(i)
        a_pose, a_proj, d_proj, a_pp, gone = absorbed_set([factors[i]._keys for i in pose_f], proj,
                                                          [factors[i]._keys[0] for i in pps], expired_keys, ts, cut)
        # cut the factor list: absorbed (the sub-graph), kept, dropped
        drop = {i: set() for i, f in enumerate(factors) if isinstance(f, _BLOCKS)}
        take = {i: [] for i in drop}
        absorbed, removed = [], set()
        for i, a in zip(pose_f, a_pose):
            if a:
                absorbed.append(factors[i]); removed.add(i)
        for i, a in zip(pps, a_pp):
            if a:
                absorbed.append(factors[i]); removed.add(i)
        for (i, r), a, dd in zip(proj_at, a_proj, d_proj):
            stats["discarded_factors"] += int(dd and not a)
            if r < 0:
                if a:
                    absorbed.append(factors[i])
                if a or dd:
                    removed.add(i)
            else:
                if a:
                    take[i].append(r)
                if a or dd:
                    drop[i].add(r)
        kept = []
        for i, f in enumerate(factors):
            if i in drop:
                if take[i]:
                    absorbed.append(_cut_block(f, np.asarray(take[i])))
                rest = np.setdiff1d(np.arange(len(f)), np.fromiter(drop[i], np.int64, len(drop[i])))
                if len(rest):
                    kept.append(f if len(rest) == len(f) else _cut_block(f, rest))
            elif i not in removed:
                kept.append(f)
        stats.update(marginalized_landmarks=len(gone), expired_poses=n_exp,
                     absorbed_factors=sum(len(f) if isinstance(f, _BLOCKS) else 1 for f in absorbed))
        # the sub-problem: the expired poses and the kept poses up to the last one an absorbed factor touches
        touched = set()
        for f in absorbed:
            touched.update(_pose_key_of(k) for k in (f.pose_keys.tolist() if isinstance(f, _BLOCKS) else f._keys))
        idx = {int(k): j for j, k in enumerate(pose_keys.tolist())}
        last = max([idx[k] for k in touched if k in idx] + [n_exp])
        sub_pose_keys = pose_keys[:last + 1]
        sub = _g.Values()
        sub.insert_pose3_block(sub_pose_keys, theta.pose3_block(sub_pose_keys))
        if inertial:
            for p in sub_pose_keys.tolist():
                for k in keyframe_keys(p)[1:]:
                    sub.insert(k, theta._at(k, object, "at"))
        if gone:
            sub.insert_point3_block(np.asarray(gone, np.int64), theta.point3_block(np.asarray(gone, np.int64)))
        sub_graph = _g.NonlinearFactorGraph()
        for f in absorbed:
            sub_graph.push_back(f)
        import torch
        # an inertial sub-problem is packed with one bias per keyframe whatever it holds, and its band takes the 3 m - 1
        # nodes from X of the first kept keyframe to B of the last: m = last - n_exp + 1 poses' worth
        pg = _pack_graph(sub_graph, sub, self._device, per_keyframe=inertial)
        prob, sv = _build_solver(pg, self._device, min_span=last - n_exp + int(inertial))
        dev = prob.device
        on = lambda a: torch.from_numpy(a).to(dev)
        try:
            if inertial:
                W = sv.marginalize_head(on(pg["poses"]), on(pg["nav"]["vels"]), on(pg["nav"]["bias"]), on(pg["points"]), n_exp)
            else:
                W = sv.marginalize_head(on(pg["poses"]), on(pg["points"]), n_exp)
        except Exception as e:
            from ..ba import IndeterminantSystem
            if isinstance(e, IndeterminantSystem):
                if e.kind == "point":
                    k = pg["lm_keys"][e.index]
                elif e.kind == "bias":
                    k = keyframe_keys(sub_pose_keys[e.index])[2]
                else:               # a node: of an inertial window X(i), V(i), B(i) in turn
                    k = keyframe_keys(sub_pose_keys[e.index // 3])[e.index % 3] if inertial else sub_pose_keys[e.index]
                raise _g.IndeterminantLinearSystemException(int(k)) from None
            raise
        kept_keys = [int(k) for k in sub_pose_keys[n_exp:]]
        point = _g.Values()
        point.insert_pose3_block(np.asarray(kept_keys, np.int64), W.x0.cpu().numpy())
        if inertial:
            keys = [k for p in kept_keys for k in keyframe_keys(p)]
            for p, v, b in zip(kept_keys, W.v0.cpu().numpy(), W.b0.cpu().numpy()):
                point.insert(keyframe_keys(p)[1], v)
                point.insert(keyframe_keys(p)[2], _g.imuBias.ConstantBias(b[:3], b[3:]))
            hf = _g.HessianFactor._from_dense(keys, W.H.cpu().numpy(), W.g.cpu().numpy(), W.c_const, dims=[6, 3, 6] * len(kept_keys))
        else:
            hf = _g.HessianFactor._from_dense(kept_keys, W.H.cpu().numpy(), W.g.cpu().numpy(), W.c_const)
        kept.append(_g.LinearContainerFactor(hf, point))
        for k in expired_keys + list(gone):
            theta.erase(k)
            ts.pop(k, None)
        self._factors, self._theta, self._ts = kept, theta, ts
        return stats


def _cut_block(f, rows):
    """The rows `rows` of a StereoFactorBlock / ProjectionFactorBlock as a new block."""
    return type(f)(f.meas[rows], f._model, f.pose_keys[rows], f.landmark_keys[rows], f._K, f.body_P_sensor())
