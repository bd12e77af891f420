"""Plain numpy statement of vus_stereo_pair_bundle (include/vus_pair_bundle.h): the two-view refit of a loop closure, the
inlier points left free and both stereo observations (x, y, d) of every point in the sum.  Test infrastructure only (a
plain module, not a conftest).

The reference restates the header operation by operation, vectorised over the candidates of a pair with plain loops over
the rounds; candidates, tables, the 6 x 6 solve and the retraction are loop_ref's.  Its sums over the active points run in
numpy's order, so T_ab, S, chi2 and points agree with the kernel to rounding; every DECISION (a point in front of both
cameras, the gate, a 3 x 3 or 6 x 6 pivot) is the same as long as no quantity lies within rounding of its bound.  Margins
extends loop_ref.Margins by the gate test and the 3 x 3 pivots, and case() certifies each fixture: no gate test within 1e-6
relative of its bound, no pivot below 1e-9 of its diagonal entry.
"""
import numpy as np

import loop_ref as L
import subpixel_ref as SP

STATUS_OK, STATUS_FEW, STATUS_SOLVE, STATUS_PASSED = 0, 1, 3, 4


class Margins(L.Margins):
    def __init__(self):
        super().__init__()
        self.gate = np.inf         # min |e2 / gate^2 - 1| and, for the two depth tests, |z| / |point|
        self.pivot3 = np.inf       # min |d| / A[j][j] over the 3 x 3 Cholesky pivots

    def safe(self):
        return super().safe() and self.gate > L.MARGIN and self.pivot3 > L.PIVOT_MARGIN

    def __repr__(self):
        return f"Margins(gate={self.gate:.3g}, pivot3={self.pivot3:.3g}, pivot={self.pivot:.3g})"


def weights(sigma_uv_px, sigma_disp_px):
    su, sd = np.float64(sigma_uv_px), np.float64(sigma_disp_px)
    wu, wd = 1.0 / (su * su), 1.0 / (sd * sd)
    return np.array([wu, wu, wd])


def project(Y, cam):
    """(pi(Y) [n,3], D(Y) [n,3,3]) of the header: pi = (fx Yx/Yz + cx, fy Yy/Yz + cy, fb/Yz)."""
    fx, fy, cx, cy, bl = (np.float64(v) for v in cam[:5])
    fb = fx * bl
    with np.errstate(all="ignore"):
        iz = 1.0 / Y[:, 2]
        a, b, e = fx * iz, fy * iz, fb * iz
        px, py = Y[:, 0] * iz, Y[:, 1] * iz
        pi = np.stack([fx * px + cx, fy * py + cy, e], 1)
        z = np.zeros_like(a)
        D = np.stack([np.stack([a, z, -(a * px)], 1), np.stack([z, b, -(b * py)], 1), np.stack([z, z, -(e * iz)], 1)], 1)
    return pi, D


def pose_jacobian(D, X):
    """Jt = D(X) [ [X]x | -I ], [n,3,6]: the rows of loop_ref.jacobians and the disparity row under them."""
    a, b, g2, h2, k2 = D[:, 0, 0], D[:, 1, 1], D[:, 0, 2], D[:, 1, 2], D[:, 2, 2]
    z = np.zeros_like(a)
    J0 = np.stack([-(g2 * X[:, 1]), g2 * X[:, 0] - a * X[:, 2], a * X[:, 1], -a, z, -g2], 1)
    J1 = np.stack([b * X[:, 2] - h2 * X[:, 1], h2 * X[:, 0], -(b * X[:, 0]), z, -b, -h2], 1)
    J2 = np.stack([-(k2 * X[:, 1]), k2 * X[:, 0], z, z, z, -k2], 1)
    return np.stack([J0, J1, J2], 1)


def residuals(T12, p, za, zb, cam, w):
    """(ra, rb, e2, X, Da, Db) of the current state."""
    X = L.transform(T12, p)
    pa, Da = project(p, cam)
    pb, Db = project(X, cam)
    ra, rb = pa - za, pb - zb
    with np.errstate(all="ignore"):
        e2 = ((w[0] * ra[:, 0] * ra[:, 0] + w[1] * ra[:, 1] * ra[:, 1]) + w[2] * ra[:, 2] * ra[:, 2]) + \
             ((w[0] * rb[:, 0] * rb[:, 0] + w[1] * rb[:, 1] * rb[:, 1]) + w[2] * rb[:, 2] * rb[:, 2])
    return ra, rb, e2, X, Da, Db


def blocks(T12, p, za, zb, cam, w):
    """The per-point blocks of one round: dict(A [n,3,3], B [n,3,6], C [n,6,6], gp [n,3], gt [n,6], e2 [n], X [n,3])."""
    ra, rb, e2, X, Da, Db = residuals(T12, p, za, zb, cam, w)
    R = T12[:9].reshape(3, 3)
    Ja = Da
    Jp = np.einsum("nkm,cm->nkc", Db, R)                      # D(X) R^T
    Jt = pose_jacobian(Db, X)
    with np.errstate(all="ignore"):
        A = np.einsum("k,nkr,nkc->nrc", w, Ja, Ja) + np.einsum("k,nkr,nkc->nrc", w, Jp, Jp)
        B = np.einsum("k,nkr,nkc->nrc", w, Jp, Jt)
        C = np.einsum("k,nkr,nkc->nrc", w, Jt, Jt)
        gp = np.einsum("k,nkr,nk->nr", w, Ja, ra) + np.einsum("k,nkr,nk->nr", w, Jp, rb)
        gt = np.einsum("k,nkr,nk->nr", w, Jt, rb)
    return dict(A=A, B=B, C=C, gp=gp, gt=gt, e2=e2, X=X, Jt=Jt, Jp=Jp, Ja=Ja, ra=ra, rb=rb)


def cholesky3(A, mg=None):
    """(L [n,3,3], ok [n]) of A = L L^T per point; ok is false at a pivot that is not > 0."""
    n = len(A)
    Lm, ok = np.zeros((n, 3, 3)), np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(3):
            d = A[:, j, j].copy()
            for k in range(j):
                d = d - Lm[:, j, k] * Lm[:, j, k]
            if mg is not None:
                live = ok & (A[:, j, j] > 0)
                if live.any():
                    mg.pivot3 = min(mg.pivot3, float(np.abs(d[live] / A[live, j, j]).min()))
            ok &= d > 0
            Lm[:, j, j] = np.sqrt(np.where(d > 0, d, 1.0))
            for i in range(j + 1, 3):
                v = A[:, i, j].copy()
                for k in range(j):
                    v = v - Lm[:, i, k] * Lm[:, j, k]
                Lm[:, i, j] = v / Lm[:, j, j]
    return Lm, ok


def solve3(Lm, rhs):
    """A^-1 rhs per point from its Cholesky factor; rhs [n,3] or [n,3,m]."""
    r = rhs if rhs.ndim == 3 else rhs[:, :, None]
    y = np.zeros_like(r)
    for i in range(3):
        v = r[:, i].copy()
        for k in range(i):
            v = v - Lm[:, i, k, None] * y[:, k]
        y[:, i] = v / Lm[:, i, i, None]
    x = np.zeros_like(r)
    for i in (2, 1, 0):
        v = y[:, i].copy()
        for k in range(i + 1, 3):
            v = v - Lm[:, k, i, None] * x[:, k]
        x[:, i] = v / Lm[:, i, i, None]
    return x if rhs.ndim == 3 else x[:, :, 0]


def reduced(T12, p, za, zb, cam, w, gate, mg=None):
    """One pass over the points: dict(active [n] bool, S [6,6], g [6], chi2, bl the blocks, Lm, AinvB, Ainvgp)."""
    bl = blocks(T12, p, za, zb, cam, w)
    gate2 = np.float64(gate) * np.float64(gate)
    with np.errstate(all="ignore"):
        front = (p[:, 2] > 0) & (bl["X"][:, 2] > 0)
        active = front & (bl["e2"] <= gate2)
    if mg is not None and len(p):
        with np.errstate(all="ignore"):
            mz = np.minimum(np.abs(p[:, 2]) / np.maximum(np.linalg.norm(p, axis=1), 1e-300),
                            np.abs(bl["X"][:, 2]) / np.maximum(np.linalg.norm(bl["X"], axis=1), 1e-300))
            mg.gate = min([mg.gate, float(mz.min())] + ([float(np.abs(bl["e2"][front] / gate2 - 1.0).min())] if front.any() else []))
    idx = np.nonzero(active)[0]
    Lm = np.zeros((len(p), 3, 3))
    Lsub, ok = cholesky3(bl["A"][idx], mg)
    Lm[idx] = Lsub
    active[idx[~ok]] = False
    idx = np.nonzero(active)[0]
    Y, yp = np.zeros((len(p), 3, 6)), np.zeros((len(p), 3))
    Y[idx], yp[idx] = solve3(Lm[idx], bl["B"][idx]), solve3(Lm[idx], bl["gp"][idx])
    Si = bl["C"][idx] - np.einsum("nkr,nkc->nrc", bl["B"][idx], Y[idx])
    gi = bl["gt"][idx] - np.einsum("nkr,nk->nr", bl["B"][idx], yp[idx])
    S = Si.sum(0)
    S = np.triu(S) + np.triu(S, 1).T                          # the kernel sums the upper triangle and mirrors it
    return dict(active=active, S=S, g=gi.sum(0), chi2=float(bl["e2"][idx].sum()), bl=bl, Y=Y, yp=yp)


def pair_bundle(x1, y1, d1, x2, y2, d2, cam, T_in, passed, sigma_uv_px, sigma_disp_px, gate, iters, mg=None):
    """One pair: its candidates as float64 arrays in index order.  Returns dict(T [12], S [6,6], chi2, points [n,3],
    keep [n] bool, info (6 ints))."""
    za, zb = (np.stack([np.asarray(q, np.float64) for q in z], 1).reshape(-1, 3) for z in ((x1, y1, d1), (x2, y2, d2)))
    cam = np.asarray(cam, np.float64)
    n = len(za)
    Tc = np.asarray(T_in, np.float64).copy()
    out = dict(T=Tc, S=np.zeros((6, 6)), chi2=0.0, points=np.zeros((n, 3)), keep=np.zeros(n, bool))
    if passed:
        out["info"] = (0, 0, 0, STATUS_PASSED, 0, 0)
        return out
    if n < 3:
        out["info"] = (n, 0, 0, STATUS_FEW, 0, 0)
        return out
    w = weights(sigma_uv_px, sigma_disp_px)
    p = L.points(za[:, 0], za[:, 1], za[:, 2], cam)
    status, rounds, first = STATUS_OK, 0, 0
    for it in range(iters + 1):
        r = reduced(Tc, p, za, zb, cam, w, gate, mg)
        if it == 0:
            first = int(r["active"].sum())
        if it == iters:
            break
        delta = L.cholesky_solve(r["S"], r["g"], mg) if r["active"].sum() >= 3 else None
        if delta is None:
            status = STATUS_SOLVE
            break
        act = r["active"]
        # p <- p - A^-1 (gp - B delta) = p - (A^-1 gp - (A^-1 B) delta)
        step = r["yp"][act] - np.einsum("nrc,c->nr", r["Y"][act], delta)
        p = p.copy()
        p[act] = p[act] - step
        Tc = L.retract(Tc, -delta)
        rounds += 1
    out["T"] = Tc
    if status == STATUS_OK:
        out.update(S=r["S"], chi2=r["chi2"], keep=r["active"], points=np.where(r["active"][:, None], p, 0.0))
    out["info"] = (n, first, int(r["active"].sum()) if status == STATUS_OK else 0, status, rounds, 0)
    return out


def stereo_pair_bundle(t, T_in, info_in, sigma_uv_px, sigma_disp_px, gate, iters, disp_q8=None, mg=None):
    """vus_stereo_pair_bundle on a table dict whose match_idx is stage one's match_idx_out: dict(T_ab [P,12], S [P,36],
    chi2 [P], points [P,K,3], match_idx_out [P,K], info [P,6])."""
    Pn, K = t["match_idx"].shape
    res = dict(T_ab=np.zeros((Pn, 12)), S=np.zeros((Pn, 36)), chi2=np.zeros(Pn), points=np.zeros((Pn, K, 3)),
               match_idx_out=np.full((Pn, K), -1, np.int32), info=np.zeros((Pn, 6), np.int32))
    for c in range(Pn):
        src, dst, *cand = L.candidates(t, c) if disp_q8 is None else SP.candidates_q8(t, c, np.asarray(disp_q8))
        o = pair_bundle(*cand, t["cam"], T_in[c], int(info_in[c][4]) != 0, sigma_uv_px, sigma_disp_px, gate, iters, mg)
        res["T_ab"][c], res["S"][c], res["chi2"][c], res["info"][c] = o["T"], o["S"].reshape(-1), o["chi2"], o["info"]
        res["match_idx_out"][c, src[o["keep"]]] = dst[o["keep"]]
        res["points"][c, src[o["keep"]]] = o["points"][o["keep"]]
    return res


def left_refit(x1, y1, d1, x2, y2, cam, T_in, threshold_px, iters):
    """The left-image refit of vus_stereo_pair_pose alone, from T_in: what the two-view refit is measured against."""
    cam = np.asarray(cam, np.float64)
    P, u, v = L.points(x1, y1, d1, cam), np.asarray(x2, np.float64), np.asarray(y2, np.float64)
    Tc, thr2 = np.asarray(T_in, np.float64).copy(), np.float64(threshold_px) ** 2
    for _ in range(iters):
        inl, X = L.inliers(Tc, P, u, v, cam, thr2)
        if inl.sum() < 3:
            break
        H, g, _ = L.normal_equations(X[inl], u[inl], v[inl], cam)
        delta = L.cholesky_solve(H, g)
        if delta is None:
            break
        Tc = L.retract(Tc, -delta)
    return Tc


# ======================================================================================================================
# fixtures: stage one (loop_ref) on loop_ref's tables, then this stage on its outputs

SIGMA_UV, SIGMA_D, GATE, ITERS = 0.5, 0.6, 4.0, 10
# nine pairs on five frames: every frame serves three or four pairs, on either side
SHARED9 = dict(seed=68, K=512, sizes=[(40 + 5 * c, 30 - 3 * c) for c in range(9)],
               frames=[(0, 1), (1, 2), (2, 0), (0, 3), (3, 1), (2, 3), (3, 4), (4, 0), (1, 4)])
_cache = {}


def stage_one(name, n_hyp=L.N_HYP):
    """(tables whose match_idx is stage one's match_idx_out, T_in, info_in) of a loop_ref fixture."""
    if ("stage1", name, n_hyp) not in _cache:
        if name == "shared9":
            t = L.planted_tables(**SHARED9)
            t["cam"] = L.default_cam5(t["H"], t["W"])
            mg = L.Margins()
            ref = L.stereo_pair_pose(t, L.THRESHOLD, n_hyp, L.SEED, L.REFINE, mg)
            assert mg.safe(), (name, mg)
        else:
            t, ref = L.case(name, n_hyp=n_hyp)
        t2 = dict(t, match_idx=ref["match_idx_out"].copy())
        _cache["stage1", name, n_hyp] = (t2, ref["T_ab"].copy(), ref["info"].astype(np.int32).copy())
    return _cache["stage1", name, n_hyp]


def certify(key, t, T_in, info_in, sigma_uv_px=SIGMA_UV, sigma_disp_px=SIGMA_D, gate=GATE, iters=ITERS, disp_q8=None):
    """The reference's outputs on (t, T_in, info_in), built once per key and certified margin-safe."""
    key = ("case", key, sigma_uv_px, sigma_disp_px, gate, iters, disp_q8 is not None)
    if key not in _cache:
        mg = Margins()
        ref = stereo_pair_bundle(t, T_in, info_in, sigma_uv_px, sigma_disp_px, gate, iters, disp_q8, mg)
        assert mg.safe(), (key, mg)
        _cache[key] = ref
    return _cache[key]


def case(name, n_hyp=L.N_HYP, **kw):
    """(tables, T_in, info_in, the reference's outputs) of the loop_ref fixture `name` after stage one."""
    t, T_in, info_in = stage_one(name, n_hyp)
    return t, T_in, info_in, certify((name, n_hyp), t, T_in, info_in, **kw)


def explicit_case(name):
    """Small hand-made pairs: (tables, T_in, info_in, reference).  "few": n = 0..4 candidates, every one a true match of
    an exact planted pose; "gated": a live pair whose start is so far off that the gate leaves fewer than three points
    (status 3 by count) beside a good one; "passed": stage one's status is non-zero for pair 0 and zero for pair 1."""
    if ("explicit", name) in _cache:
        return _cache["explicit", name]
    H, W = 480, 640
    cam = L.default_cam5(H, W)
    Tp = L.pose12((0.0, 0.02, 0.1), (0.2, 0.0, 0.0))
    if name == "few":
        rng = np.random.default_rng(71)
        sizes = [0, 1, 2, 3, 4]
        pairs = [(2 * c, 2 * c + 1, L.planted_pair(rng, n, 0, Tp, H, W, zrange=(1.5, 2.5))) for c, n in enumerate(sizes)]
        t = L.tables_from_pairs(rng, pairs, 2 * len(sizes), 40, H, W)
        T_in = np.tile(Tp, (len(sizes), 1))
        info_in = np.zeros((len(sizes), 6), np.int32)
    elif name == "gated":
        rng = np.random.default_rng(72)
        pairs = [(0, 1, L.planted_pair(rng, 40, 0, Tp, H, W, zrange=(1.5, 2.5))),
                 (2, 3, L.planted_pair(rng, 40, 0, Tp, H, W, zrange=(1.5, 2.5)))]
        t = L.tables_from_pairs(rng, pairs, 4, 64, H, W)
        T_in = np.stack([L.pose12((0.0, 0.02, 0.1), (0.8, 0.3, 0.0)), Tp])     # 0.6 m off: every point fails the gate
        info_in = np.zeros((2, 6), np.int32)
    elif name == "passed":
        rng = np.random.default_rng(73)
        pairs = [(0, 1, L.planted_pair(rng, 40, 0, Tp, H, W, zrange=(1.5, 2.5))),
                 (1, 2, L.planted_pair(rng, 40, 0, Tp, H, W, zrange=(1.5, 2.5)))]
        t = L.tables_from_pairs(rng, pairs, 3, 128, H, W)
        T_in = np.stack([L.pose12((0.3, 0.1, 0.2), (1.0, 2.0, 3.0)), Tp])
        info_in = np.array([[40, -1, -1, 0, 2, 0], [40, 3, 40, 40, 0, 10]], np.int32)
    else:
        raise KeyError(name)
    t["cam"] = cam
    _cache["explicit", name] = (t, T_in, info_in, certify(("explicit", name), t, T_in, info_in))
    return _cache["explicit", name]


def degenerate_tables(name):
    """Collinear or duplicate points: S is singular, its later pivots are rounding errors of either sign, so no reference
    can be certified; the kernel test holds these to what is true whichever way a rounding error falls."""
    H, W = 480, 640
    rng = np.random.default_rng(74)
    if name == "collinear":
        rows = [(100 + 9 * q, 200, 24, 90 + 9 * q, 200, 24) for q in range(40)]
    else:
        rows = [(300, 240, 20, 310, 240, 20)] * 12
    t = L.tables_from_pairs(rng, [(0, 1, L._explicit(rng, rows))], 2, 64, H, W)
    t["cam"] = L.default_cam5(H, W)
    r = rows[0]
    T_in = L.IDENTITY12.copy()
    T_in[9] = (r[0] - r[3]) * L.BASELINE / r[2]               # the shift in x that maps b's points onto a's
    return t, T_in[None], np.zeros((1, 6), np.int32)
