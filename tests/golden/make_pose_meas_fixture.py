#!/usr/bin/env python3
"""Generate tests/golden/pose_meas_general_position.npz: position and attitude fixes on poses (include/vus_pose_meas.h)
in general position with a 60-digit reference and a per-block error bound derived from that reference alone, by the rule
of make_general_position.py, whose mpmath helpers it imports (run from the repo root:
python tests/golden/make_pose_meas_fixture.py; needs mpmath, a few seconds, no GPU and no oracle library).

The reference states both factors from first principles in mpmath and shares no formula, branch or threshold with the
kernels or the numpy reference.  The f64 inputs are taken exactly as given; only Log projects its argument onto SO(3)
first (se3_log of make_general_position.py).
  POSITION   r = W (t + R a - m), the STATED J = W [ -R [a]x , R ]
  ROTATION   r = W Log(Rm^T R),   the STATED J = W [ I , 0 ]  (not the true derivative by design, as gtsam has it)
  the robust table of include/vus_robust.h per factor; the Hpp / gp increments and the error of vus_pose_meas_linearize,
  the two scalars of vus_pose_meas_eval_step at a stored step and stored new poses, vus_pose_meas_error, and the
  weights of vus_pose_meas_weights in CSR order.

The case: 8 poses uniform on SO(3) a kilometre from the origin; 12 position and 12 rotation factors in a graph order that
is not sorted by pose; rotation residuals of 1e-9 rad, of general size and of pi - 1e-3; lever arms up to a metre (and
none); sigmas spanning 1e-2 .. 1e3 within one factor; each of the six losses on a factor of either kind on either side of
its threshold, with the generator's 1e-6 relative margin from every discontinuity (it asserts; choose another seed if it
fires); pose 3 carries five factors of both kinds and pose 6 none.

Bounds: tol_block = 32 * (largest change of the block under 8 seeded draws of every input double times 1 +- 2^-53)
+ 32 * 2^-53 * max|block| (with_bounds of make_general_position.py).  `oracle_ratio_<array>` records the worst
|numpy reference - want| / tol_block of tests/pose_meas_ref.py when the file was made (tests/test_pose_meas_ref.py
recomputes it and bounds it by 1)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_general_position import (with_bounds, se3_exp, robust, se3_log, rows, rot, trans, mul, hat, tangent, angle,  # noqa: E402
                                   random_rotation, f64_pose, save, MARGIN)
from mpmath import mpf, matrix, sqrt  # noqa: E402
from general_position import ratios  # noqa: E402

SEED = 20261019
N_POSES = 8
ROT_ANGLES = ["1e-9", "0.3", "pi-1e-3", "1", "2.5", "1e-9", "pi-1e-3", "0.05", "1.7", "1e-9", "pi-1e-3", "0.6"]
FLOAT_INPUTS = ["poses", "meas", "w", "loss_k", "dp", "new_poses"]
OUTPUTS = ["Hpp", "gp", "err", "eval", "error", "weights"]


def factor(kind, m9, w3, T):
    """(unwhitened r [3], J [3][6], d2) of one factor at the pose T, in mpmath"""
    R, t = rot(T), trans(T)
    if kind == 1:
        Rm = rot(m9)
        r = se3_log(Rm.T * R, matrix([0, 0, 0]))[:3]
        J = [[mpf(1) if c == a else mpf(0) for c in range(6)] for a in range(3)]
    else:
        m, a = matrix(m9[0:3]), matrix(m9[3:6])
        v = t + R * a - m
        r = [v[0], v[1], v[2]]
        A = -(R * hat(a))
        J = [[A[x, c] for c in range(3)] + [R[x, c] for c in range(3)] for x in range(3)]
    d2 = sum((w3[x] * r[x]) ** 2 for x in range(3))
    return r, J, d2


def reference(I):
    """Every output of the case with inputs I (mpf rows / int arrays), as a dict of lists of blocks (flat mpf lists)."""
    nP, n = len(I["poses"]), len(I["idx"])
    Hpp = [[mpf(0)] * 36 for _ in range(nP)]
    gp = [[mpf(0)] * 6 for _ in range(nP)]
    err, e_lin, e_new, e_at, wts = mpf(0), mpf(0), mpf(0), mpf(0), {}
    for f in range(n):
        i, kind, lk, k = int(I["idx"][f]), int(I["kind"][f]), int(I["loss_kind"][f]), I["loss_k"][f][0]
        w3 = I["w"][f]
        r, J, d2 = factor(kind, I["meas"][f], w3, I["poses"][i])
        w, rho = robust(lk, k, d2)
        w2 = [w * w3[x] ** 2 for x in range(3)]
        for a in range(6):
            for c in range(6):
                Hpp[i][6 * a + c] += sum(J[x][a] * w2[x] * J[x][c] for x in range(3))
            gp[i][a] += sum(J[x][a] * w2[x] * r[x] for x in range(3))
        err += w * d2 / 2
        e_at += rho
        wts[f] = w
        d = I["dp"][i]
        e_lin += sum(w2[x] * (r[x] + sum(J[x][c] * d[c] for c in range(6))) ** 2 for x in range(3)) / 2
        _, _, d2n = factor(kind, I["meas"][f], w3, I["new_poses"][i])
        e_new += robust(lk, k, d2n)[1]
    order = np.argsort(np.asarray(I["idx"]), kind="stable")
    return {"Hpp": Hpp, "gp": gp, "err": [[err]], "eval": [[e_lin], [e_new]], "error": [[e_at]],
            "weights": [[wts[int(f)]] for f in order]}


def to_mp(I, rng=None):
    M = dict(I)
    for key in FLOAT_INPUTS:
        M[key] = rows(I[key], rng)
    return M


def case(seed=SEED):
    rng = np.random.default_rng(seed)
    nP = N_POSES
    poses = np.zeros((nP, 12))
    for i in range(nP):
        p = rng.standard_normal(3)
        poses[i] = np.concatenate([random_rotation(rng).reshape(-1), 1000.0 * p / np.linalg.norm(p) + rng.uniform(-5, 5, 3)])
    Pm = rows(poses)
    n_pos = n_rot = 12
    n = n_pos + n_rot
    # graph position f -> pose: five factors of both kinds on pose 3, none on pose 6, the rest spread in a scrambled order
    on3 = {0, 7, 13, 20, 22}
    others = [5, 0, 7, 2, 4, 1]
    idx = np.array([3 if f in on3 else others[(5 * f + f // 6) % 6] for f in range(n)], np.int32)
    assert (idx == 3).sum() == 5 and not (idx == 6).any() and len(set(idx.tolist())) == 7 and (np.diff(idx) < 0).any()
    kind = np.array([0] * n_pos + [1] * n_rot, np.int32)
    assert set(kind[idx == 3].tolist()) == {0, 1}
    meas, sig = np.zeros((n, 9)), np.zeros((n, 3))
    for f in range(n):
        i = int(idx[f])
        R, t = rot(Pm[i]), trans(Pm[i])
        if kind[f] == 0:
            sig[f] = [1e-2, 1.0, 1e3] if f == 3 else 10.0 ** rng.uniform(-2, 3, 3) if f % 3 == 0 else rng.uniform(0.05, 2.0, 3)
            arm = np.zeros(3) if f % 4 == 0 else rng.uniform(-1, 1, 3) / np.sqrt(3.0)
            noise = sig[f] * rng.standard_normal(3)
            a = matrix([mpf(float(x)) for x in arm])
            m = t + R * a + matrix([mpf(float(x)) for x in noise])
            meas[f] = [float(m[0]), float(m[1]), float(m[2]), *arm, 0.0, 0.0, 0.0]
        else:
            sig[f] = [1e-2, 1.0, 1e3] if f == 15 else rng.uniform(0.01, 0.3, 3)
            Re, _ = se3_exp(tangent(rng, angle(ROT_ANGLES[f - n_pos]), 0))
            Rm = R * Re.T                                  # Rm^T R = Exp(xi): the residual has the named angle
            meas[f] = [float(Rm[a, c]) for a in range(3) for c in range(3)]
    w = 1.0 / sig
    loss_kind = np.array([f % 6 for f in range(n)], np.int32)
    # k on either side of the whitened residual norm: factors 0-5 and 12-17 are outliers of their loss (k = 0.4 d),
    # factors 6-11 and 18-23 inliers (k = 2.5 d); a Gaussian factor ignores it
    loss_k = np.ones(n)
    Mm, Wm = rows(meas), rows(w)
    for f in range(n):
        _, _, d2 = factor(int(kind[f]), Mm[f], Wm[f], Pm[int(idx[f])])
        d = float(sqrt(d2))
        assert d > 0.0
        loss_k[f] = 1.0 if loss_kind[f] == 0 else d * (0.4 if (f // 6) % 2 == 0 else 2.5)
    dp = np.array([[float(x) for x in tangent(rng, mpf("0.05"), mpf("0.5"))] for _ in range(nP)])
    new = []
    for i in range(nP):
        Re, te = se3_exp([mpf(float(x)) * mpf("0.3") for x in dp[i]])
        new.append(f64_pose(*mul(rot(Pm[i]), trans(Pm[i]), Re, te)))
    return {"poses": poses, "idx": idx, "kind": kind, "meas": meas, "sigmas": sig, "w": w, "loss_kind": loss_kind,
            "loss_k": loss_k.reshape(-1, 1), "dp": dp, "new_poses": np.array(new)}


def numpy_outputs(c):
    """The outputs of the case from the numpy reference tests/pose_meas_ref.py, in the fixture's block shapes."""
    import pose_meas_ref as pmr
    G = pmr.PoseMeasSet(c["idx"], c["kind"], c["meas"], c["sigmas"], list(zip(c["loss_kind"].tolist(), c["loss_k"].reshape(-1).tolist())))
    H, g, e, fac = pmr.blocks(G, c["poses"])
    return {"Hpp": H, "gp": g, "err": np.array([[e]]),
            "eval": np.array([[pmr.linear_error(fac, c["dp"])], [pmr.error(G, c["new_poses"])]]),
            "error": np.array([[pmr.error(G, c["poses"])]]), "weights": pmr.weights(G, c["poses"])[G.csr_order()].reshape(-1, 1)}


def main():
    c = case()
    c.update(with_bounds(dict(c), SEED, reference, to_mp))
    for k, v in ratios(numpy_outputs(c), c, OUTPUTS).items():
        c["oracle_ratio_" + k] = np.float64(v)
        print(f"pose_meas {k:8s} numpy reference / tol = {v:.3g}")
    path = os.path.join(HERE, "pose_meas_general_position.npz")
    save(path, c)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 100000 and MARGIN == 1e-6


if __name__ == "__main__":
    main()
