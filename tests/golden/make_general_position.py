#!/usr/bin/env python3
"""Generate tests/golden/general_position_*.npz: the bundle-adjustment factors in general position with a 60-digit
reference and a per-block error bound derived from that reference alone (run from the repo root:
python tests/golden/make_general_position.py [case ...]; needs mpmath and the built CPU oracle, about three minutes).

The reference states each factor from first principles in mpmath and shares no formula, branch or threshold with the
kernels or the oracle.  The f64 inputs are taken exactly as given: the 12 doubles of a pose are used as they are (its
inverse is (R^T, -R^T t), what every pose kernel means by it); only Log projects its argument onto SO(3) first (polar
factor), since the logarithm of a matrix that is orthonormal to 1e-16 only is otherwise not defined.

  Log       angle atan2(|v| / 2, (tr - 1) / 2) and axis v / |v| of the projected rotation (v its antisymmetric part; at 60
            digits this is accurate to 1e-40 for every angle of the cases), translation V(omega)^-1 t by a linear solve
  Exp       I + sin th / th W + (1 - cos th) / th^2 W^2 and V = I + (1 - cos th) / th^2 W + (th - sin th) / th^3 W^2
  BetweenFactorPose3   r = Log(meas^-1 T1^-1 T2), the STATED H1 = -Ad(hx^-1), H2 = I (include/vus_between.h), the
            robust table of include/vus_robust.h; the 120-double record and error of vus_between_linearize, the two
            scalars of vus_between_eval_step
  PriorFactorPose3     r = -W Log(T^-1 prior), the STATED H = I: Hpp, gp and the error of vus_ba_linearize on a graph
            without observations; new_poses = T Exp(dp), the linear and the new error of vus_ba_eval_step
  stereo / mono projection, PriorFactorPoint3   (uL, uR, v) of the stereo camera and (u, v) of the pinhole camera with skew
            at the camera pose X o body_P_sensor, the cheirality rule z <= 0 of ba.hip, whitening, the six losses;
            W, V, gl, Hpp, gp, the errors, the weights and eval_step at a stored step, once per loss kind
  ImuFactor, DVL, velocity prior   the residuals of nav.hip over a preintegration record taken as data; Snav, Scb, Sbb,
            gnav, gb and the error of vus_nav_linearize (shared-bias layout), the outputs of vus_nav_eval_step
The projection, point-prior, ImuFactor and DVL Jacobians are central differences of the residual through the retraction
T Exp(xi) with a step of 1e-20 (accurate to 1e-40): no analytic derivative is written down here.  The pose prior and the
between factor are NOT the true derivative by design (gtsam's defaults); their stated formulas are evaluated.

Bounds (float32, one per block: an 18-vector of W, a V, a 6 x 6 of Hpp / Snav, a 120-record, a pose, a scalar ...):
the reference is evaluated again at the inputs with every double multiplied by 1 +- 2^-53 (8 seeded draws); the largest
change of any element of the block is what rounding the inputs alone causes, and
    tol_block = FACTOR * that + FACTOR * 2^-53 * max|block|,   FACTOR = 32
(a handful of fixed-order sums per block, and the final roundings).  The generator asserts a relative margin of 1e-6 from
every discontinuity (the cheirality plane, Huber d = k, Tukey d^2 = k^2, rotation by pi): choose another seed if it fires.

Each file also records `oracle_ratio_<array>`: the worst |oracle - want| / tol_block of the f64 CPU twins when the file
was made (tests/test_general_position.py recomputes it and bounds it by 1).  Some inputs (the new poses a between
evaluation reads, the preintegration records) are made by the oracle and stored: they are data to the reference."""
import os
import sys

import numpy as np
from mpmath import mp, mpf, matrix, sqrt, sin, cos, atan2, log, exp, pi, lu_solve, eye

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from general_position import oracle_outputs, ratios  # noqa: E402  (tests/general_position.py: no mpmath there)

mp.dps = 60
FACTOR = 32
DRAWS = 8
EPS = 2.0 ** -53
MARGIN = 1e-6

# |omega| of the residuals and steps: 0, below the th < 1e-10 switch of Pose3::Logmap, both sides of th2 <= kEps (1.49e-8), of the th2 < 1e-10 switch of the SO(3)
# Jacobians, of the tr - 3 < -1e-7 switch of Log (3.16e-4), mid range, and the band towards pi
ANGLES = ["0", "5e-11", "1e-9", "1.4e-8", "1.6e-8", "9e-6", "1.1e-5", "3.0e-4", "3.3e-4", "1", "2.5",
          "pi-1e-2", "pi-1e-3", "pi-1e-4", "pi-2e-5", "pi-9e-6", "pi-5e-6"]


def angle(s):
    return pi - mpf(s[3:]) if s.startswith("pi-") else mpf(s)


# ---- SE(3) in mpmath ------------------------------------------------------------------------------------------------
def hat(w):
    return matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def rot(T):
    return matrix([[T[0], T[1], T[2]], [T[3], T[4], T[5]], [T[6], T[7], T[8]]])


def trans(T):
    return matrix([T[9], T[10], T[11]])


def inv(R, t):
    return R.T, -(R.T * t)


def mul(Ra, ta, Rb, tb):
    return Ra * Rb, ta + Ra * tb


def so3_coeffs(th):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3); series below 1e-20, where 60 digits would cancel."""
    if th < mpf("1e-20"):
        return 1 - th * th / 6, mpf(1) / 2 - th * th / 24, mpf(1) / 6 - th * th / 120
    return sin(th) / th, (1 - cos(th)) / (th * th), (th - sin(th)) / (th ** 3)


def se3_exp(xi):
    w, v = matrix(xi[:3]), matrix(xi[3:])
    th = sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    a, b, c = so3_coeffs(th)
    W = hat(w)
    return eye(3) + a * W + b * W * W, (eye(3) + b * W + c * W * W) * v


def polar(R, iters=8):
    """The rotation nearest to R (orthogonal polar factor) by Newton's iteration (quadratic: 1e-16 -> 1e-32 -> 1e-64)."""
    X = R.copy()
    for _ in range(iters):
        X = (X + (X ** -1).T) / 2
    return X


def se3_log(R, t, iters=8):
    Q = polar(R, iters)
    v = matrix([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    nv = sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    th = atan2(nv / 2, (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1) / 2)
    assert pi - th > MARGIN * pi, "a rotation within the margin of pi: re-draw the seed"
    w = v * (th / nv) if nv > 0 else matrix([0, 0, 0])
    _, b, c = so3_coeffs(th)
    W = hat(w)
    u = lu_solve(eye(3) + b * W + c * W * W, t)
    return [w[0], w[1], w[2], u[0], u[1], u[2]]


def adjoint(R, t):
    A = matrix(6, 6)
    tR = hat(t) * R
    for r in range(3):
        for c in range(3):
            A[r, c] = A[3 + r, 3 + c] = R[r, c]
            A[3 + r, c] = tR[r, c]
    return A


def robust(kind, k, d2):
    """(w, rho) of include/vus_robust.h at the squared whitened norm d2."""
    d = sqrt(d2)
    if kind == 0:
        return mpf(1), d2 / 2
    k2 = k * k
    if kind == 1:
        assert abs(d - k) > MARGIN * k, "Huber d = k within the margin: re-draw the seed"
        return (mpf(1), d2 / 2) if d <= k else (k / d, k * d - k2 / 2)
    if kind == 2:
        return k2 / (k2 + d2), k2 / 2 * log(1 + d2 / k2)
    if kind == 3:
        assert abs(d2 - k2) > MARGIN * k2, "Tukey d^2 = k^2 within the margin: re-draw the seed"
        t = 1 - d2 / k2
        return (t * t, k2 / 6 * (1 - t ** 3)) if d2 <= k2 else (mpf(0), k2 / 6)
    if kind == 4:
        return k2 * k2 / (k2 + d2) ** 2, k2 / 2 * d2 / (k2 + d2)
    if kind == 5:
        return exp(-d2 / k2), k2 / 2 * (1 - exp(-d2 / k2))
    raise ValueError(kind)


# ---- the outputs of the entry points, in mpmath ----------------------------------------------------------------------
def between_factor(T1, T2, M, w6, kind, k):
    """(r, H1, w, rho, d2) of one BetweenFactorPose3 (H2 = I)."""
    Rh, th = mul(*inv(rot(T1), trans(T1)), rot(T2), trans(T2))
    r = se3_log(*mul(*inv(rot(M), trans(M)), Rh, th))
    H1 = -adjoint(*inv(Rh, th))
    d2 = sum((w6[a] * r[a]) ** 2 for a in range(6))
    w, rho = robust(kind, k, d2)
    return r, H1, w, rho, d2


def pose_reference(I):
    """Every output of a pose case with inputs I (a dict of mpf lists / int arrays), as a dict of flat mpf lists."""
    poses, nP = I["poses"], len(I["poses"])
    out = {}
    # BetweenFactorPose3
    lin, err, e_lin, e_new = [], mpf(0), mpf(0), mpf(0)
    for f in range(len(I["btw_i"])):
        a, b = int(I["btw_i"][f]), int(I["btw_j"][f])
        kind, k, w6 = int(I["btw_kind"][f]), I["btw_k"][f], I["btw_w"][f]
        r, H1, w, rho, d2 = between_factor(poses[a], poses[b], I["btw_meas"][f], w6, kind, k)
        w2 = [w * w6[q] ** 2 for q in range(6)]
        rec = [sum(H1[q, x] * w2[q] * H1[q, y] for q in range(6)) for x in range(6) for y in range(6)]
        rec += [H1[y, x] * w2[y] for x in range(6) for y in range(6)]
        rec += [w2[x] if x == y else mpf(0) for x in range(6) for y in range(6)]
        rec += [sum(H1[q, x] * w2[q] * r[q] for q in range(6)) for x in range(6)]
        rec += [w2[x] * r[x] for x in range(6)]
        lin.append(rec)
        err += w * d2 / 2
        d1, dd2 = I["dp"][a], I["dp"][b]
        for q in range(6):
            v = r[q] + sum(H1[q, x] * d1[x] for x in range(6)) + dd2[q]
            e_lin += w2[q] * v * v / 2
        _, _, _, rho_new, _ = between_factor(I["btw_new_poses"][a], I["btw_new_poses"][b], I["btw_meas"][f], w6, kind, k)
        e_new += rho_new
    out["btw_lin"], out["btw_err"], out["btw_eval"] = lin, [[err]], [[e_lin], [e_new]]
    # PriorFactorPose3 on a graph without observations, and the retraction
    Hpp = [[mpf(0)] * 36 for _ in range(nP)]
    gp = [[mpf(0)] * 6 for _ in range(nP)]
    new_poses, err, e_lin, e_new = [], mpf(0), mpf(0), mpf(0)
    for i in range(nP):
        Re, te = se3_exp(I["dp"][i])
        Rn, tn = mul(rot(poses[i]), trans(poses[i]), Re, te)
        new_poses.append([Rn[r, c] for r in range(3) for c in range(3)] + [tn[0], tn[1], tn[2]])
    for q in range(len(I["prior_pose"])):
        i, w6, Tp = int(I["prior_pose"][q]), I["prior_w"][q], I["prior_T"][q]
        xi = se3_log(*mul(*inv(rot(poses[i]), trans(poses[i])), rot(Tp), trans(Tp)))
        xn = se3_log(*mul(*inv(rot(new_poses[i]), trans(new_poses[i])), rot(Tp), trans(Tp)))
        for a in range(6):
            r = -xi[a] * w6[a]
            Hpp[i][7 * a] += w6[a] ** 2
            gp[i][a] += w6[a] * r
            err += r * r / 2
            e_lin += (r + w6[a] * I["dp"][i][a]) ** 2 / 2
            e_new += (xn[a] * w6[a]) ** 2 / 2
    out["Hpp"], out["gp"], out["err"], out["new_poses"], out["eval"] = Hpp, gp, [[err]], new_poses, [[e_lin], [e_new]]
    return out


# ---- projection factors in mpmath (poses as (R [9], t [3]) lists: plain arithmetic, no matrix objects) ---------------------
H_STEP = mpf("1e-20")          # central differences at 60 digits: truncation 1e-40, cancellation leaves 40 digits


def compose(X, S):
    """X o S for poses given as 12 mpf (R row-major, then t)."""
    if S is None:
        return list(X)
    R = [sum(X[3 * r + k] * S[3 * k + c] for k in range(3)) for r in range(3) for c in range(3)]
    return R + [X[9 + r] + sum(X[3 * r + k] * S[9 + k] for k in range(3)) for r in range(3)]


def retracted(X, xi):
    """X Exp(xi) as 12 mpf."""
    Re, te = se3_exp(xi)
    return compose(X, [Re[r, c] for r in range(3) for c in range(3)] + [te[0], te[1], te[2]])


def camera_z(C, p):
    return sum(C[3 * k + 2] * (p[k] - C[9 + k]) for k in range(3))


def residual_rows(C, p, m, cal, mono):
    """The three whitened rows of one observation of point p from the CAMERA pose C: (uL, uR, v) - m of the stereo camera
    cal = (fx, fy, cx, cy, b, w), or rows 0 and 2 = (u, v) - (m0, m2) of the pinhole camera cal = (fx, fy, s, cx, cy, w)
    with row 1 zero.  Camera-frame z <= 0 (the rule documented in ba.hip): 2 fx w on every row the factor has."""
    d = [p[k] - C[9 + k] for k in range(3)]
    x, y, z = [C[c] * d[0] + C[3 + c] * d[1] + C[6 + c] * d[2] for c in range(3)]
    assert z == 0 or abs(z) > MARGIN * sqrt(x * x + y * y + z * z), "within the margin of the cheirality plane: re-draw"
    if mono:
        fx, fy, sk, cx, cy, w = cal
        if z <= 0:
            return [2 * fx * w, mpf(0), 2 * fx * w]
        return [(cx + (fx * x + sk * y) / z - m[0]) * w, mpf(0), (cy + fy * y / z - m[2]) * w]
    fx, fy, cx, cy, b, w = cal
    if z <= 0:
        return [2 * fx * w] * 3
    return [(cx + fx * x / z - m[0]) * w, (cx + fx * (x - b) / z - m[1]) * w, (cy + fy * y / z - m[2]) * w]


def proj_reference(I):
    """Every output of a projection case, per loss kind (suffix _k<kind>) where the loss enters."""
    S = I["sensor"][0] if len(I["sensor"]) else None
    poses, points, nP, nL, nO = I["poses"], I["points"], len(I["poses"]), len(I["points"]), len(I["obs_pose"])
    stereo = [I["K"][0][0], I["K"][0][1], I["K"][0][3], I["K"][0][4], I["K"][0][5], I["inv_sigma"][0][0]]
    pin = I["mono_K"][0] + [I["mono_w"][0][0]]
    e6 = [[H_STEP if a == k else mpf(0) for a in range(6)] for k in range(6)]
    cams = [compose(X, S) for X in poses]
    cams_p = [[compose(retracted(X, e6[k]), S) for k in range(6)] for X in poses]
    cams_m = [[compose(retracted(X, [-v for v in e6[k]]), S) for k in range(6)] for X in poses]
    new_poses = [retracted(poses[i], I["dp"][i]) for i in range(nP)]
    new_cams = [compose(X, S) for X in new_poses]
    new_points = [[points[j][c] + I["dl"][j][c] for c in range(3)] for j in range(nL)]
    fac = []
    for a in range(nO):
        i, j, m, mono = int(I["obs_pose"][a]), int(I["obs_point"][a]), I["meas"][a], bool(I["is_mono"][a])
        cal, p = pin if mono else stereo, points[j]
        r = residual_rows(cams[i], p, m, cal, mono)
        H1 = [[mpf(0)] * 6 for _ in range(3)]
        H2 = [[mpf(0)] * 3 for _ in range(3)]
        # a cheirality observation has zero Jacobians by the stated rule (on the plane itself there is no derivative)
        cheiral = r[0] == r[2] == 2 * cal[0] * cal[-1] and camera_z(cams[i], p) <= 0
        for k in range(0 if cheiral else 6):
            rp, rm = residual_rows(cams_p[i][k], p, m, cal, mono), residual_rows(cams_m[i][k], p, m, cal, mono)
            for row in range(3):
                H1[row][k] = (rp[row] - rm[row]) / (2 * H_STEP)
        for c in range(0 if cheiral else 3):
            pp, pm = list(p), list(p)
            pp[c] += H_STEP
            pm[c] -= H_STEP
            rp, rm = residual_rows(cams[i], pp, m, cal, mono), residual_rows(cams[i], pm, m, cal, mono)
            for row in range(3):
                H2[row][c] = (rp[row] - rm[row]) / (2 * H_STEP)
        rn = residual_rows(new_cams[i], new_points[j], m, cal, mono)
        t = [r[row] + sum(H1[row][k] * I["dp"][i][k] for k in range(6)) + sum(H2[row][c] * I["dl"][j][c] for c in range(3))
             for row in range(3)]
        fac.append((i, j, r, H1, H2, sum(v * v for v in r), sum(v * v for v in rn), sum(v * v for v in t)))
    # PriorFactorPoint3: r = w (p - mean), J = diag(w), never reweighted
    ppV, ppg = [[mpf(0)] * 6 for _ in range(nL)], [[mpf(0)] * 3 for _ in range(nL)]
    pp_err = pp_new = mpf(0)
    for q in range(len(I["pp_idx"])):
        j = int(I["pp_idx"][q])
        for c, slot in enumerate((0, 3, 5)):
            w = I["pp_w"][q][c]
            ppV[j][slot] += w * w
            ppg[j][c] += w * w * (points[j][c] - I["pp_mean"][q][c])
            pp_err += (w * (points[j][c] - I["pp_mean"][q][c])) ** 2 / 2
            pp_new += (w * (new_points[j][c] - I["pp_mean"][q][c])) ** 2 / 2
    out = {"new_poses": new_poses, "new_points": new_points, "pp_err": [[pp_err]], "pp_eval": [[pp_new], [pp_new]]}
    tri = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for kind, k in zip(I["loss_kind"], I["loss_k"]):
        kind, k = int(kind), k[0]
        W, wts = [], []
        V, gl = [list(v) for v in ppV], [list(v) for v in ppg]
        Hpp, gp = [[mpf(0)] * 36 for _ in range(nP)], [[mpf(0)] * 6 for _ in range(nP)]
        err = error = e_lin = e_new = mpf(0)
        for i, j, r, H1, H2, d2, d2n, t2 in fac:
            w, rho = robust(kind, k, d2)
            W.append([w * sum(H1[row][x] * H2[row][y] for row in range(3)) for x in range(6) for y in range(3)])
            wts.append([w])
            for slot, (x, y) in enumerate(tri):
                V[j][slot] += w * sum(H2[row][x] * H2[row][y] for row in range(3))
            for x in range(3):
                gl[j][x] += w * sum(H2[row][x] * r[row] for row in range(3))
            for x in range(6):
                gp[i][x] += w * sum(H1[row][x] * r[row] for row in range(3))
                for y in range(6):
                    Hpp[i][6 * x + y] += w * sum(H1[row][x] * H1[row][y] for row in range(3))
            err += w * d2 / 2
            error += rho
            e_lin += w * t2 / 2
            e_new += robust(kind, k, d2n)[1]
        for name, v in (("W", W), ("weights", wts), ("V", V), ("gl", gl), ("Hpp", Hpp), ("gp", gp), ("err", [[err]]),
                        ("error", [[error]]), ("eval", [[e_lin], [e_new]])):
            out[f"{name}_k{kind}"] = v
    return out


PROJ_FLOAT_INPUTS = ["poses", "points", "meas", "K", "inv_sigma", "mono_K", "mono_w", "sensor", "pp_mean", "pp_w", "dp", "dl",
                     "loss_k"]


def proj_to_mp(I, rng=None):
    M = dict(I)
    for key in PROJ_FLOAT_INPUTS:
        M[key] = rows(I[key], rng)
    return M


# ---- inertial factors in mpmath -----------------------------------------------------------------------------------------
PIM = dict(DT=0, DR=1, DP=10, DV=13, DR_DBG=16, DP_DBA=25, DP_DBG=34, DV_DBA=43, DV_DBG=52, BIAS=61, COV=67, N=148)


def mat3(v, o=0):
    return matrix([[v[o], v[o + 1], v[o + 2]], [v[o + 3], v[o + 4], v[o + 5]], [v[o + 6], v[o + 7], v[o + 8]]])


def imu_residual(Ti, vi, Tj, vj, bias, pim, g):
    """ImuFactor (nav.hip / Forster et al. 2017) over the preintegration record pim, taken as data: with the bias deltas
    dba, dbg from the record's bias,  dRc = dR Exp(dR_dbg dbg),  dPc = dP + dP_dba dba + dP_dbg dbg,  dVc likewise,
      r = ( Log(Rj^T Ri dRc),  Rj^T (p_i + v_i dt + g dt^2 / 2 + Ri dPc - p_j),  Rj^T (v_i + g dt + Ri dVc - v_j) )."""
    dt = pim[PIM["DT"]]
    dba = matrix([bias[k] - pim[PIM["BIAS"] + k] for k in range(3)])
    dbg = matrix([bias[3 + k] - pim[PIM["BIAS"] + 3 + k] for k in range(3)])
    phi = mat3(pim, PIM["DR_DBG"]) * dbg
    dRc = mat3(pim, PIM["DR"]) * se3_exp([phi[0], phi[1], phi[2], 0, 0, 0])[0]
    dPc = matrix(pim[PIM["DP"]:PIM["DP"] + 3]) + mat3(pim, PIM["DP_DBA"]) * dba + mat3(pim, PIM["DP_DBG"]) * dbg
    dVc = matrix(pim[PIM["DV"]:PIM["DV"] + 3]) + mat3(pim, PIM["DV_DBA"]) * dba + mat3(pim, PIM["DV_DBG"]) * dbg
    Ri, pi_, Rj, pj = rot(Ti), trans(Ti), rot(Tj), trans(Tj)
    vi, vj, g = matrix(vi), matrix(vj), matrix(g)
    rR = se3_log(Rj.T * Ri * dRc, matrix([0, 0, 0]), iters=4)[:3]
    rP = Rj.T * (pi_ + vi * dt + g * (dt * dt / 2) + Ri * dPc - pj)
    rV = Rj.T * (vi + g * dt + Ri * dVc - vj)
    return rR + [rP[0], rP[1], rP[2], rV[0], rV[1], rV[2]]


def dvl_residual(T, v, m):
    """DVL velocity factor: R m - v (the body-frame measurement turned into the world frame against the velocity)."""
    Rm = rot(T) * matrix(m)
    return [Rm[k] - v[k] for k in range(3)]


def differences(f, args, slots):
    """d f / d (slots) by central differences: slots = [(argument index, 'pose' | 'vec', size)], a pose through its
    retraction T Exp(xi); returns J[row][column]."""
    cols = []
    for a, how, n in slots:
        for k in range(n):
            out = []
            for sgn in (1, -1):
                moved = list(args)
                if how == "pose":
                    moved[a] = retracted(args[a], [sgn * H_STEP if q == k else mpf(0) for q in range(6)])
                else:
                    moved[a] = [x + (sgn * H_STEP if q == k else 0) for q, x in enumerate(args[a])]
                out.append(f(*moved))
            cols.append([(x - y) / (2 * H_STEP) for x, y in zip(*out)])
    return [[cols[c][r] for c in range(len(cols))] for r in range(len(cols[0]))]


def nav_reference(I):
    """The outputs of vus_nav_linearize and vus_nav_eval_step (shared-bias layout: node 2i = pose i, node 2i + 1 =
    velocity i padded to 6, the bias a border)."""
    poses, vels, bias, g, nP = I["poses"], I["vels"], I["bias"][0], I["gravity"][0], len(I["poses"])
    nN = 2 * nP
    facs = []                                  # (whitened J rows, whitened r, [(node, dim)] per column; node -1 = the bias)
    for f in range(len(I["imu_i"])):
        i, j, pim = int(I["imu_i"][f]), int(I["imu_j"][f]), I["imu_pim"][f]
        args = [poses[i], vels[i], poses[j], vels[j], bias, pim, g]
        r = imu_residual(*args)
        J = differences(imu_residual, args, [(0, "pose", 6), (1, "vec", 3), (2, "pose", 6), (3, "vec", 3), (4, "vec", 6)])
        W = [I["imu_W"][f][9 * a:9 * a + 9] for a in range(9)]
        cols = [(2 * i, d) for d in range(6)] + [(2 * i + 1, d) for d in range(3)] + [(2 * j, d) for d in range(6)] + \
               [(2 * j + 1, d) for d in range(3)] + [(-1, d) for d in range(6)]
        facs.append(([[sum(W[a][q] * J[q][c] for q in range(9)) for c in range(24)] for a in range(9)],
                     [sum(W[a][q] * r[q] for q in range(9)) for a in range(9)], cols,
                     lambda P, V, B, i=i, j=j, pim=pim, W=W: [sum(W[a][q] * x for q, x in enumerate(
                         imu_residual(P[i], V[i], P[j], V[j], B, pim, g))) for a in range(9)]))
    for f in range(len(I["dvl_pose"])):
        i, m, w = int(I["dvl_pose"][f]), I["dvl_meas"][f], I["dvl_w"][f][0]
        args = [poses[i], vels[i], m]
        r = dvl_residual(*args)
        J = differences(dvl_residual, args, [(0, "pose", 6), (1, "vec", 3)])
        facs.append(([[w * x for x in row] for row in J], [w * x for x in r],
                     [(2 * i, d) for d in range(6)] + [(2 * i + 1, d) for d in range(3)],
                     lambda P, V, B, i=i, m=m, w=w: [w * x for x in dvl_residual(P[i], V[i], m)]))
    for f in range(len(I["vp_idx"])):
        i, v0, w3 = int(I["vp_idx"][f]), I["vp_v"][f], I["vp_w"][f]
        facs.append(([[w3[a] if a == c else mpf(0) for c in range(3)] for a in range(3)],
                     [w3[a] * (vels[i][a] - v0[a]) for a in range(3)], [(2 * i + 1, d) for d in range(3)],
                     lambda P, V, B, i=i, v0=v0, w3=w3: [w3[a] * (V[i][a] - v0[a]) for a in range(3)]))
    Snav = [[mpf(0)] * 36 for _ in range(4 * nN)]
    Scb, gnav = [[mpf(0)] * 36 for _ in range(nN)], [[mpf(0)] * 6 for _ in range(nN)]
    Sbb, gb, err, e_lin = [mpf(0)] * 36, [mpf(0)] * 6, mpf(0), mpf(0)
    for Jw, rw, cols, _ in facs:
        err += sum(x * x for x in rw) / 2
        step = [I["db"][0][d] if n < 0 else I["dc"][n][d] for n, d in cols]
        e_lin += sum((rw[a] + sum(Jw[a][c] * step[c] for c in range(len(cols)))) ** 2 for a in range(len(rw))) / 2
        for c1, (n1, d1) in enumerate(cols):
            gsum = sum(Jw[a][c1] * rw[a] for a in range(len(rw)))
            if n1 < 0:
                gb[d1] += gsum
            else:
                gnav[n1][d1] += gsum
            for c2, (n2, d2) in enumerate(cols):
                h = sum(Jw[a][c1] * Jw[a][c2] for a in range(len(rw)))
                if n1 < 0 and n2 < 0:
                    Sbb[6 * d1 + d2] += h
                elif n2 < 0:
                    Scb[n1][6 * d1 + d2] += h
                elif n1 >= n2 >= 0:
                    Snav[4 * n1 + (n1 - n2)][6 * d1 + d2] += h
    new_vels = [[vels[i][k] + I["dc"][2 * i + 1][k] for k in range(3)] for i in range(nP)]
    new_bias = [bias[k] + I["db"][0][k] for k in range(6)]
    e_new = sum(sum(x * x for x in at(I["new_poses"], new_vels, new_bias)) for _, _, _, at in facs) / 2
    return {"Snav": Snav, "Scb": Scb, "Sbb": [Sbb], "gnav": gnav, "gb": [gb], "nav_err": [[err]], "new_vels": new_vels,
            "new_bias": [new_bias], "nav_eval": [[e_lin], [e_new]]}


NAV_FLOAT_INPUTS = ["poses", "vels", "bias", "gravity", "imu_pim", "imu_W", "dvl_meas", "dvl_w", "vp_v", "vp_w", "dc", "db",
                    "new_poses"]


def nav_to_mp(I, rng=None):
    M = dict(I)
    for key in NAV_FLOAT_INPUTS:
        M[key] = rows(I[key], rng)
    return M


POSE_FLOAT_INPUTS = ["poses", "btw_meas", "btw_w", "btw_k", "btw_new_poses", "dp", "prior_T", "prior_w"]


def rows(a, rng=None):
    """A f64 array [n, ...] as n rows of mpf, exactly; with rng every double is multiplied by 1 +- 2^-53 first."""
    a = np.asarray(a, np.float64)
    a = a.reshape(len(a), a.size // max(len(a), 1))
    s = np.zeros(a.shape, np.int64) if rng is None else rng.integers(0, 2, a.shape) * 2 - 1
    return [[mpf(float(a[r, c])) * (1 + int(s[r, c]) * mpf(2) ** -53 if rng is not None else 1) for c in range(a.shape[1])]
            for r in range(a.shape[0])]


def pose_to_mp(I, rng=None):
    """The inputs of a pose case with its f64 arrays as mpf (index arrays stay as they are)."""
    M = dict(I)
    for key in POSE_FLOAT_INPUTS:
        M[key] = rows(I[key], rng)
    M["btw_k"] = [row[0] for row in M["btw_k"]]
    return M


def rounded(blocks):
    return np.array([[float(x) for x in b] for b in blocks], np.float64)


def with_bounds(I, seed, reference, to_mp):
    """want_<array> (f64, rounded once) and tol_<array> (float32, one per block) of the case."""
    want = reference(to_mp(I))
    rng = np.random.default_rng(seed)
    change = {k: [mpf(0)] * len(want[k]) for k in want}
    for _ in range(DRAWS):
        got = reference(to_mp(I, rng))
        for k in want:
            for b in range(len(want[k])):
                change[k][b] = max([change[k][b]] + [abs(x - y) for x, y in zip(got[k][b], want[k][b])])
    out = {}
    for k in want:
        out["want_" + k] = rounded(want[k])
        tol = [FACTOR * change[k][b] + FACTOR * EPS * max([abs(x) for x in want[k][b]] + [mpf(0)]) for b in range(len(want[k]))]
        out["tol_" + k] = np.array([float(t) for t in tol], np.float32)
        # float32 rounds to nearest: never store a bound below the derived one
        low = out["tol_" + k].astype(np.float64) < np.array([float(t) for t in tol])
        out["tol_" + k][low] = np.nextafter(out["tol_" + k][low], np.float32(np.inf))
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    """Uniform on SO(3) (a normalised Gaussian quaternion), rounded to f64."""
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def tangent(rng, ang, tscale):
    """xi (mpf) with |omega| = ang exactly (to 60 digits) on a generic axis and a translation part of size tscale."""
    ax = rng.standard_normal(3)
    ax = [mpf(float(x)) for x in ax]
    n = sqrt(sum(x * x for x in ax))
    return [ang * x / n for x in ax] + [mpf(float(x)) * tscale for x in rng.standard_normal(3)]


def f64_pose(R, t):
    return np.array([float(R[r, c]) for r in range(3) for c in range(3)] + [float(t[0]), float(t[1]), float(t[2])])


def lie_edges(seed, own):
    """8 poses uniform on SO(3) in a 10 m ball (pose 0 = the identity, so that one relative pose is exact), a between
    factor for every angle of ANGLES (residual rotation = the angle, translations up to 1e3, each loss kind on both sides
    of k), a pose prior on every pose and a step for every pose whose |omega| are the 8 angles `own`."""
    rng = np.random.default_rng(seed)
    nP = 8
    poses = np.zeros((nP, 12))
    poses[0, [0, 4, 8]] = 1.0
    for i in range(1, nP):
        p = rng.standard_normal(3)
        poses[i] = np.concatenate([random_rotation(rng).reshape(-1), 10.0 * rng.uniform() ** (1 / 3) * p / np.linalg.norm(p)])
    Pm = rows(poses)
    scales = [1, 1000, 10, 1, 100]
    pairs = [(0, 1), (6, 3), (3, 1), (2, 7), (5, 4), (1, 2), (6, 2), (4, 7), (7, 3), (2, 0), (3, 4), (5, 6), (6, 1), (0, 5), (4, 2),
             (7, 5), (1, 6)]
    meas, kinds, ks, sig = [], [], [], []
    for f, (name, (a, b)) in enumerate(zip(ANGLES, pairs)):
        Rh, th = mul(*inv(rot(Pm[a]), trans(Pm[a])), rot(Pm[b]), trans(Pm[b]))
        if name == "0":
            Rm, tm = Rh, th                    # exact in f64: pose a is the identity
        else:                                  # meas = hx Exp(xi)^-1, so that Log(meas^-1 hx) = xi
            Re, te = se3_exp(tangent(rng, angle(name), scales[f % 5]))
            Rm, tm = mul(Rh, th, *inv(Re, te))
        meas.append(f64_pose(Rm, tm))
        sig.append(np.concatenate([rng.uniform(0.01, 0.1, 3), rng.uniform(0.05, 0.5, 3)]))
        kinds.append(f % 6)
    w = 1.0 / np.array(sig)
    # k on either side of the whitened residual norm, alternating per kind (a Gaussian factor ignores it)
    I0 = {"poses": poses, "btw_i": np.array([p[0] for p in pairs], np.int32), "btw_j": np.array([p[1] for p in pairs], np.int32),
          "btw_meas": np.array(meas), "btw_w": w}
    for f in range(len(pairs)):
        _, _, _, _, d2 = between_factor(Pm[pairs[f][0]], Pm[pairs[f][1]], rows(I0["btw_meas"])[f], rows(w)[f], 0, mpf(1))
        d = float(sqrt(d2))
        ks.append(1.0 if kinds[f] == 0 else max(d, 0.5) * (0.4 if (f // 6) % 2 == 0 else 2.5))
    # steps and priors: prior = pose Exp(xi) with |omega| = the angle, step dp with the same |omega| on another axis
    dp, prior_T, psig = [], [], []
    for i, name in enumerate(own):
        dp.append([float(x) for x in tangent(rng, angle(name), scales[(i + 2) % 5])])
        if name == "0":
            prior_T.append(poses[i].copy())
        else:
            Re, te = se3_exp(tangent(rng, angle(name), scales[i % 5]))
            prior_T.append(f64_pose(*mul(rot(Pm[i]), trans(Pm[i]), Re, te)))
        psig.append(np.concatenate([rng.uniform(0.01, 0.1, 3), rng.uniform(0.05, 0.5, 3)]))
    dp = np.array(dp)
    from oracle import oracle as O              # the new poses the between eval reads are INPUT data: any nearby poses do
    new = np.stack([O.pose_retract(poses[i], 0.3 * dp[i] / max(1.0, np.abs(dp[i]).max())) for i in range(nP)])
    I0.update(btw_kind=np.array(kinds, np.int32), btw_k=np.array(ks), btw_sigma=np.array(sig), btw_new_poses=new, dp=dp,
              prior_pose=np.arange(nP, dtype=np.int32), prior_T=np.array(prior_T), prior_sigma=np.array(psig),
              prior_w=1.0 / np.array(psig))
    return I0


def np_compose(X, S):
    R, t = X[:9].reshape(3, 3), X[9:]
    return X if S is None else np.concatenate([(R @ S[:9].reshape(3, 3)).reshape(-1), t + R @ S[9:]])


def np_camera_point(C, p):
    return C[:9].reshape(3, 3).T @ (p - C[9:])


def projection_graph(seed, K, sigma, S=None, mono_frac=0.0, mono_K=None, mono_sigma=1.0, n_point_priors=0, offset=None):
    """6 poses uniform on SO(3) in a 10 m ball (pose 0 = the identity at the origin), 24 landmarks, each in front of its 1-5
    observers at a depth log-uniform in 0.3-200 m; measurements = the f64 projection + 1 px of noise, every tenth row
    50-300 px off.  Landmark 0: z = 0 exactly in camera 0 (without an extrinsic) next to ordinary sightings; landmark 1:
    behind one of its cameras; landmark 2: behind all of them; landmark 3: a single sighting; landmark 4 (with mono rows):
    mono sightings only.  Rows are in L-order (by landmark, then pose).  `offset` translates poses and points afterwards
    (and lifts landmark 0 off the plane of camera 0: after the translation an exact zero would sit within rounding of the
    discontinuity, which no bound can judge)."""
    rng = np.random.default_rng(seed)
    nP, nL = 6, 24
    poses = np.zeros((nP, 12))
    poses[0, [0, 4, 8]] = 1.0
    for i in range(1, nP):
        v = rng.standard_normal(3)
        poses[i] = np.concatenate([random_rotation(rng).reshape(-1), 10.0 * rng.uniform() ** (1 / 3) * v / np.linalg.norm(v)])
    cams = np.stack([np_compose(X, S) for X in poses])
    front = lambda p, i: (lambda q: q[2] > 0.05 * np.linalg.norm(q))(np_camera_point(cams[i], p))
    behind = lambda p, i: (lambda q: q[2] < -0.05 * np.linalg.norm(q))(np_camera_point(cams[i], p))
    points, obs = np.zeros((nL, 3)), []
    for j in range(nL):
        while True:
            i0 = 0 if j == 0 else int(rng.integers(nP))
            depth = float(np.exp(rng.uniform(np.log(0.3), np.log(200.0))))
            q = depth * np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
            if j == 0:
                q = np.array([0.7, -0.4, 0.0]) if S is None else np.array([0.7, -0.4, 1.5])
            if j == 2:
                q = -q
            p = cams[i0, :9].reshape(3, 3) @ q + cams[i0, 9:]
            others = [i for i in range(nP) if i != i0 and (behind(p, i) if j == 2 else front(p, i))]
            want = {0: 2, 1: 2, 2: 1, 3: 0}.get(j, j % 5)
            back = [i for i in range(nP) if i != i0 and behind(p, i)]
            if len(others) >= min(want, 1) and (j != 1 or back) and (j in (0, 2) or front(p, i0)):
                break
        seen = [i0] + [int(i) for i in rng.permutation(others)[:want]] + ([back[0]] if j == 1 else [])
        points[j] = p
        obs += [(j, i) for i in sorted(seen)]
    obs_point, obs_pose = np.array([o[0] for o in obs], np.int32), np.array([o[1] for o in obs], np.int32)
    nO = len(obs)
    is_mono = (rng.uniform(size=nO) < mono_frac).astype(np.uint8)
    if mono_frac:
        is_mono[obs_point == 4] = 1
        is_mono[obs_point == 0] = 0
    fx, fy, _, cx, cy, b = K
    meas = np.zeros((nO, 3))
    for a in range(nO):
        x, y, z = np_camera_point(cams[obs_pose[a]], points[obs_point[a]])
        if z <= 0.0:
            meas[a] = rng.uniform(0.0, 600.0, 3)
        elif is_mono[a]:
            meas[a] = [mono_K[3] + (mono_K[0] * x + mono_K[2] * y) / z, rng.uniform(0.0, 600.0), mono_K[4] + mono_K[1] * y / z]
        else:
            meas[a] = [cx + fx * x / z, cx + fx * (x - b) / z, cy + fy * y / z]
        meas[a] += rng.standard_normal(3)
        if a % 10 == 7:
            meas[a, int(rng.integers(3))] += rng.choice([-1.0, 1.0]) * rng.uniform(50.0, 300.0)
    dp = np.concatenate([0.02 * rng.standard_normal((nP, 3)), 0.05 * rng.standard_normal((nP, 3))], 1)
    dl = 0.03 * rng.standard_normal((nL, 3)) * np.linalg.norm(points, axis=1)[:, None].clip(0.3, 30.0)
    dp[0] = 0.0                 # pose 0 and landmark 0 stay put: the exact zero is exact at the new values too
    dl[0] = 0.0
    pp_idx = np.array([5, 1, 5][:n_point_priors], np.int32)
    pp_sig = np.array([[0.05, 0.7, 5.0], [2.0, 0.1, 0.4], [0.7, 5.0, 0.05]][:n_point_priors]).reshape(-1, 3)
    pp_mean = points[pp_idx] + rng.standard_normal((len(pp_idx), 3)) * pp_sig
    if offset is not None:
        points[0] += cams[0, :9].reshape(3, 3) @ np.array([0.0, 0.0, 1.5])
        poses[:, 9:] += offset
        points += offset
        pp_mean = pp_mean + offset
    I = {"poses": poses, "points": points, "obs_pose": obs_pose, "obs_point": obs_point, "meas": meas, "is_mono": is_mono,
         "K": np.array([K], np.float64), "sigma": np.array([[sigma]]), "inv_sigma": np.array([[1.0 / sigma]]),
         "mono_K": np.array([mono_K if mono_K is not None else [1.0, 1.0, 0.0, 0.0, 0.0]], np.float64),
         "mono_sigma": np.array([[mono_sigma]]), "mono_w": np.array([[1.0 / mono_sigma]]),
         "sensor": np.zeros((0, 12)) if S is None else np.array([S]), "pp_idx": pp_idx, "pp_mean": pp_mean.reshape(-1, 3),
         "pp_sigma": pp_sig, "pp_w": 1.0 / pp_sig, "dp": dp, "dl": dl}
    # one loss of every kind, k = the median whitened residual norm: residuals on both sides of it
    M = proj_to_mp(I | {"loss_kind": np.zeros(1, np.int32), "loss_k": np.ones((1, 1))})
    d = np.sort(np.sqrt(2.0 * np.array([float(x[0]) for x in _per_factor_rho(M)])))
    k = float(np.round(0.5 * (d[len(d) // 2 - 1] + d[len(d) // 2]), 3))
    I["loss_kind"], I["loss_k"] = np.arange(6, dtype=np.int32), np.full((6, 1), k)
    return I


def _per_factor_rho(M):
    """Gaussian rho = d^2 / 2 of every observation (to place k)."""
    S = M["sensor"][0] if len(M["sensor"]) else None
    stereo = [M["K"][0][0], M["K"][0][1], M["K"][0][3], M["K"][0][4], M["K"][0][5], M["inv_sigma"][0][0]]
    pin = M["mono_K"][0] + [M["mono_w"][0][0]]
    out = []
    for a in range(len(M["obs_pose"])):
        mono = bool(M["is_mono"][a])
        r = residual_rows(compose(M["poses"][int(M["obs_pose"][a])], S), M["points"][int(M["obs_point"][a])], M["meas"][a],
                          pin if mono else stereo, mono)
        out.append([sum(v * v for v in r) / 2])
    return out


def _extrinsic():
    import sensor_ref
    return sensor_ref.extrinsic()


def inertial(seed, n_kf, rot_residuals, gyro_deltas):
    """n_kf keyframes with general attitudes, velocities of about 1 m/s and a gravity along no axis; ImuFactor f joins
    keyframes f and f + 1 over a record made by vus_imu_preintegrate_cpu from seeded samples with the bias estimate
    bias - (acc delta, gyro_deltas[f]); pose f + 1 is placed so that the rotation residual has the size rot_residuals[f];
    DVL factors on all keyframes, a velocity prior on the first."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v)
    g = np.array([0.6, -1.1, -9.7])
    bias = np.concatenate([0.05 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)])
    poses, vels = np.zeros((n_kf, 12)), np.zeros((n_kf, 3))
    poses[0] = np.concatenate([random_rotation(rng).reshape(-1), 5.0 * rng.standard_normal(3)])
    vels[0] = rng.standard_normal(3)
    pims, Ws = [], []
    for f in range(n_kf - 1):
        smp = np.concatenate([rng.standard_normal((10, 3)) + [0.0, 0.0, 9.8], 0.3 * rng.standard_normal((10, 3)),
                              np.full((10, 1), 0.05)], 1)
        delta = np.concatenate([(0.02 if gyro_deltas[f] else 0.0) * unit(rng.standard_normal(3)),
                                gyro_deltas[f] * unit(rng.standard_normal(3))])
        pim = O.imu_preintegrate(smp, bias - delta, 1e-4 * np.eye(3), 1e-6 * np.eye(3), 1e-8 * np.eye(3))
        if not gyro_deltas[f]:
            pim[PIM["BIAS"]:PIM["BIAS"] + 6] = bias                 # a bias delta of exactly zero
        pims.append(pim)
        Ws.append(O.sqrt_information(pim[PIM["COV"]:PIM["COV"] + 81].reshape(9, 9)).reshape(-1))
        dt, dR = pim[PIM["DT"]], pim[PIM["DR"]:PIM["DR"] + 9].reshape(3, 3)
        Ri, pi_ = poses[f, :9].reshape(3, 3), poses[f, 9:]
        ang = rot_residuals[f]
        w = float(angle(ang)) * unit(rng.standard_normal(3)) if ang != "0" else np.zeros(3)
        Rj = Ri @ dR @ O.so3_expmap(w).T                           # about Log(Rj^T Ri dR) = w (the bias correction moves it a little)
        pj = pi_ + vels[f] * dt + 0.5 * g * dt * dt + Ri @ pim[PIM["DP"]:PIM["DP"] + 3] + 0.1 * rng.standard_normal(3)
        vels[f + 1] = vels[f] + g * dt + Ri @ pim[PIM["DV"]:PIM["DV"] + 3] + 0.05 * rng.standard_normal(3)
        poses[f + 1] = np.concatenate([Rj.reshape(-1), pj])
    dvl_meas = np.stack([poses[i, :9].reshape(3, 3).T @ vels[i] for i in range(n_kf)]) + 0.05 * rng.standard_normal((n_kf, 3))
    dvl_sigma = rng.uniform(0.05, 0.2, n_kf)
    vp_sigma = np.array([[0.1, 0.3, 0.05]])
    dc = np.zeros((2 * n_kf, 6))
    dc[0::2] = np.concatenate([0.02 * rng.standard_normal((n_kf, 3)), 0.05 * rng.standard_normal((n_kf, 3))], 1)
    dc[1::2, :3] = 0.05 * rng.standard_normal((n_kf, 3))
    db = np.concatenate([0.01 * rng.standard_normal(3), 0.002 * rng.standard_normal(3)])[None]
    new_poses = np.stack([O.pose_retract(poses[i], dc[2 * i]) for i in range(n_kf)])      # INPUT of vus_nav_eval_step
    return {"poses": poses, "vels": vels, "bias": bias[None], "gravity": g[None], "imu_i": np.arange(n_kf - 1, dtype=np.int32),
            "imu_j": np.arange(1, n_kf, dtype=np.int32), "imu_pim": np.array(pims), "imu_W": np.array(Ws),
            "dvl_pose": np.arange(n_kf, dtype=np.int32), "dvl_meas": dvl_meas, "dvl_sigma": dvl_sigma[:, None],
            "dvl_w": 1.0 / dvl_sigma[:, None], "vp_idx": np.zeros(1, np.int32), "vp_v": vels[:1] + 0.05, "vp_sigma": vp_sigma,
            "vp_w": 1.0 / vp_sigma, "dc": dc, "db": db, "new_poses": new_poses}


FAR = np.array([4.1e5, 5.2e6, -3e3])
K_PLAIN = (520.0, 520.0, 0.0, 320.0, 240.0, 0.12)
K_CAL = (611.3, 587.9, 0.0, 402.6, 191.2, 0.6)
MONO_CAL = dict(mono_frac=0.4, mono_K=(455.2, 471.8, 3.7, 310.4, 255.9), mono_sigma=0.8, n_point_priors=3)

POSE_CASES = {"lie_edges_a": lambda: lie_edges(20261018, ANGLES[:1] + ANGLES[2:6] + ANGLES[11:14]),
              "lie_edges_b": lambda: lie_edges(20261019, ANGLES[6:11] + ANGLES[14:])}
PROJ_CASES = {"attitudes": lambda: projection_graph(11, K_PLAIN, 2.0),
              "attitudes_sensor": lambda: projection_graph(12, K_PLAIN, 2.0, S=_extrinsic()),
              "far_origin": lambda: projection_graph(11, K_PLAIN, 2.0, offset=FAR),
              "far_origin_sensor": lambda: projection_graph(12, K_PLAIN, 2.0, S=_extrinsic(), offset=FAR),
              "calibration": lambda: projection_graph(13, K_CAL, 0.3, **MONO_CAL),
              "calibration_sensor": lambda: projection_graph(14, K_CAL, 0.3, S=_extrinsic(), **MONO_CAL)}
# inertial: the issue's 4 keyframes (rotation residuals 0.5 and pi - 1e-3, gyro-bias deltas 0, 1e-6 and 0.05 rad/s);
# inertial_edges: rotation residuals and phi = dR_dbg dbg (about 0.5 s x the gyro delta) on either side of the th2 < 1e-10
# switch of so3_jr / so3_jr_inv and of th2 <= kEps
NAV_CASES = {"inertial": lambda: inertial(31, 4, ["0.5", "pi-1e-3", "1e-2"], [0.0, 1e-6, 0.05]),
             "inertial_edges": lambda: inertial(32, 8, ["9e-6", "1.1e-5", "0", "1.4e-8", "1.6e-8", "2.5", "pi-2e-5"],
                                                [1.8e-5, 2.2e-5, 2.8e-8, 3.2e-8, 1e-3, 0.0, 0.3])}
CASES = {**POSE_CASES, **PROJ_CASES, **NAV_CASES}


def build_case(name):
    I = CASES[name]()
    out = dict(I)
    family = (proj_reference, proj_to_mp) if name in PROJ_CASES else (nav_reference, nav_to_mp) if name in NAV_CASES else \
        (pose_reference, pose_to_mp)
    out.update(with_bounds(I, sum(map(ord, name)), *family))
    return out


def save(path, arrays):
    """An .npz whose bytes depend on the arrays alone (numpy's savez stamps every member with the time of day)."""
    import zipfile
    with zipfile.ZipFile(path, "w") as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(2026, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main(names):
    from oracle import oracle as O
    for name in names or CASES:
        c = build_case(name)
        for k, v in ratios(oracle_outputs(O, c), c).items():
            c["oracle_ratio_" + k] = np.float64(v)
            print(f"{name:18s} {k:14s} oracle / tol = {v:.3g}")
        path = os.path.join(HERE, f"general_position_{name}.npz")
        save(path, c)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < 349157


if __name__ == "__main__":
    main(sys.argv[1:])
