"""gtsam.Marginals on the MI355X: marginal covariances of the graphs the optimiser supports, from the selected inversion
of the reduced camera system's band (ba.py marginals(), include/vus_marginals.h).  GTSAM's names and semantics:
Pose3 6 x 6 in the tangent order (rot, trans) of the body frame, Point3 3 x 3 in the world frame, velocity 3 x 3,
ConstantBias 6 x 6 (acc, gyro); joint blocks in ascending key order."""
from typing import Dict, List

import numpy as np

from . import symbol_shorthand as _sym
from .optimizer import _pack_graph, _build_solver


class IndeterminantLinearSystemException(RuntimeError):
    """The information matrix at the given values is not positive definite (gtsam's exception of that name); `key` is
    the variable it was detected at."""

    def __init__(self, key, detail=""):
        self.key = int(key)
        name = _sym.key_string(self.key)
        super().__init__(f"Indeterminant linear system detected while working near variable {name} "
                         f"(Symbol: {name}).{(' ' + detail) if detail else ''}")


class KeyVector(list):
    """gtsam.KeyVector: a list of keys."""


class JointMarginal:
    """gtsam.JointMarginal: blocks of a joint covariance (or information) matrix in ascending key order."""

    def __init__(self, keys: List[int], dims: List[int], full: np.ndarray):
        self._keys, self._dims, self._full = list(keys), list(dims), full
        off = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        self._slot = {k: (int(off[i]), int(off[i + 1])) for i, k in enumerate(self._keys)}

    def at(self, key1, key2) -> np.ndarray:
        a, b = self._slot[int(key1)], self._slot[int(key2)]
        return self._full[a[0]:a[1], b[0]:b[1]].copy()

    def fullMatrix(self) -> np.ndarray:
        return self._full.copy()

    def keys(self) -> KeyVector:
        return KeyVector(self._keys)


class Marginals:
    """gtsam.Marginals(graph, values[, factorization]): linearises the graph at `values` (which need not be an optimum)
    with no damping and computes every marginal on the GPU at construction."""

    class Factorization:
        CHOLESKY = 0
        QR = 1

    CHOLESKY, QR = Factorization.CHOLESKY, Factorization.QR
    _bias_keys: List[int] = []          # one bias per keyframe: B(i) of keyframe i (empty on the other graphs)
    _bias_idx: Dict[int, int] = {}

    def __init__(self, graph, values, factorization=None, device="cuda:0"):
        import torch
        from .. import _lib
        from ..ba import IndeterminantSystem
        if factorization not in (None, Marginals.CHOLESKY):
            raise NotImplementedError("Marginals: only the CHOLESKY factorization is implemented")
        _lib.require_gpu()
        pg = _pack_graph(graph, values, device)
        nav = pg.get("nav")
        aux = pg["aux"]
        if nav and aux.keys:
            raise NotImplementedError("prior factors on extra vector variables next to inertial factors are not supported")
        prob, sv = _build_solver(pg, device)
        dev = prob.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self._pose_keys = [int(k) for k in np.asarray(pg["pose_keys"]).tolist()]
        self._lm_keys = [int(k) for k in np.asarray(pg["lm_keys"].cpu() if hasattr(pg["lm_keys"], "cpu") else pg["lm_keys"]).tolist()]
        self._vel_keys = [int(k) for k in nav["vel_keys"]] if nav else []
        self._bias_key = int(nav["bias_key"]) if nav and nav["bias_key"] is not None else None
        self._bias_keys = [int(k) for k in nav["bias_keys"]] if nav and nav.get("per_keyframe") else []
        try:
            if nav:
                m = sv.marginals(t(pg["poses"]), t(nav["vels"]), t(nav["bias"]), t(pg["points"]))
            else:
                m = sv.marginals(t(pg["poses"]), t(pg["points"]))
        except IndeterminantSystem as e:
            raise IndeterminantLinearSystemException(self._key_of(e.kind, e.index)) from None
        self._m, self._stride = m, prob.pose_stride
        self._pose_cov = m.pose_cov.cpu().numpy()
        self._point_cov = m.point_cov.cpu().numpy() if m.point_cov is not None else np.zeros((0, 3, 3))
        self._vel_cov = m.vel_cov.cpu().numpy() if m.vel_cov is not None else None
        self._bias_cov = m.bias_cov.cpu().numpy() if m.bias_cov is not None else None
        self._biases_cov = m.biases_cov.cpu().numpy() if m.biases_cov is not None else None
        self._aux: Dict[int, np.ndarray] = {int(k): np.diag(1.0 / np.asarray(w, float) ** 2) for k, w in zip(aux.keys, aux.w)}
        self._pose_idx = {k: i for i, k in enumerate(self._pose_keys)}
        self._lm_idx = {k: j for j, k in enumerate(self._lm_keys)}
        self._vel_idx = {k: i for i, k in enumerate(self._vel_keys)}
        self._bias_idx = {k: i for i, k in enumerate(self._bias_keys)}

    def _key_of(self, kind, index):
        if kind == "point":
            return self._lm_keys[index]
        if kind == "bias":
            if self._bias_keys:                      # one bias per keyframe: the index is the keyframe's
                return self._bias_keys[index]
            return self._bias_key if self._bias_key is not None else -1
        ps = (3 if self._bias_keys else 2) if self._vel_keys else 1
        i, r = divmod(index, ps)
        return (self._pose_keys, self._vel_keys, self._bias_keys)[r][i]

    def _missing(self, key):
        return RuntimeError(f"Attempting to at the key \"{_sym.key_string(int(key))}\", which does not exist in the Values.")

    def marginalCovariance(self, key) -> np.ndarray:
        key = int(key)
        if key in self._pose_idx:
            return self._pose_cov[self._pose_idx[key]].copy()
        if key in self._lm_idx:
            return self._point_cov[self._lm_idx[key]].copy()
        if key in self._vel_idx:
            return self._vel_cov[self._vel_idx[key]].copy()
        if self._bias_key is not None and key == self._bias_key:
            return self._bias_cov.copy()
        if key in self._bias_idx:
            return self._biases_cov[self._bias_idx[key]].copy()
        if key in self._aux:
            return self._aux[key].copy()
        raise self._missing(key)

    def marginalInformation(self, key) -> np.ndarray:
        return np.linalg.inv(self.marginalCovariance(key))

    def jointMarginalCovariance(self, keys) -> JointMarginal:
        keys = sorted({int(k) for k in keys})
        for k in keys:
            self.marginalCovariance(k)      # unknown keys raise as in marginalCovariance
        if len(keys) == 1:
            c = self.marginalCovariance(keys[0])
            return JointMarginal(keys, [c.shape[0]], c)
        cam = [k for k in keys if k in self._pose_idx or k in self._vel_idx or k in self._bias_idx]
        lms = [k for k in keys if k in self._lm_idx]
        nodes = [self._stride * self._pose_idx[k] if k in self._pose_idx else
                 self._stride * self._vel_idx[k] + 1 if k in self._vel_idx else self._stride * self._bias_idx[k] + 2
                 for k in cam]
        with_bias = self._bias_key is not None and self._bias_key in keys
        if lms:
            # from the band: landmarks need every pose observing them inside one band window with the other keys
            try:
                J = self._m.joint_full(nodes, [self._lm_idx[k] for k in lms], bias=with_bias)
            except NotImplementedError as e:
                raise NotImplementedError("jointMarginalCovariance of " + ", ".join(_sym.key_string(k) for k in keys) +
                                          ": " + str(e)) from None
        elif cam or with_bias:
            J = self._m.joint(nodes, bias=with_bias)
        else:
            J = np.zeros((0, 0))
        # rows of the joint for every key: a velocity node keeps its 3 real coordinates
        where = {}
        for x, k in enumerate(cam):
            d = 3 if k in self._vel_idx else 6
            where[k] = list(range(6 * x, 6 * x + d))
        if with_bias:
            where[self._bias_key] = list(range(6 * len(cam), 6 * len(cam) + 6))
        r_lm = 6 * len(cam) + 6 * with_bias
        for t, k in enumerate(lms):
            where[k] = list(range(r_lm + 3 * t, r_lm + 3 * t + 3))
        dims = []
        for k in keys:
            dims.append(len(where[k]) if k in where else self._aux[k].shape[0])
        full = np.zeros((sum(dims), sum(dims)))
        off = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        for a, ka in enumerate(keys):
            for b, kb in enumerate(keys):
                if ka in where and kb in where:
                    blk = J[np.ix_(where[ka], where[kb])]
                elif ka == kb:
                    blk = self._aux[ka]
                else:
                    blk = np.zeros((dims[a], dims[b]))          # a prior-only vector variable decouples from the rest
                full[off[a]:off[a + 1], off[b]:off[b + 1]] = blk
        return JointMarginal(keys, dims, full)

    def jointMarginalInformation(self, keys) -> JointMarginal:
        J = self.jointMarginalCovariance(keys)
        return JointMarginal(J._keys, J._dims, np.linalg.inv(J._full))
