"""Plain numpy statement of vus_stereo_pair_pose (include/vus_loop.h) and the generators of the tables it is tested on.
Test infrastructure only (a plain module, not a conftest).

The reference half restates the header statement for statement: float64 arrays combined in the header's order, the hash
in Python integers, vectorised over the candidates of a pair with plain loops over hypotheses and refit rounds.  Its
sums over the inliers run in numpy's order and its retraction uses numpy's sin / cos, so T_ab, JtJ and rss agree with
the kernel to rounding, not bit for bit; every DECISION (degenerate sample, inlier, best hypothesis, pivot) is the same
as long as no quantity lies within rounding of its bound.  The reference therefore records the margin of every decision
it takes (`Margins`), and case() certifies each fixture: no inlier test within 1e-6 relative of its threshold, no sample
within 1e-6 relative of the degeneracy bound, no pivot below 1e-9 of its diagonal entry (a refit round with fewer than
three inliers fails by count, before any pivot).

The generator half builds planted stereo pairs (a pose, points in front of camera a, projected into both rigs, rounded to
integer pixels and integer disparities, wrong matches shuffled in) and packs them into match / stereo / key tables.
"""
import numpy as np

import track_ref as T
from ransac_ref import BORDER, decode, mix, rodrigues

BASELINE = 0.063            # batch.py:110
MARGIN = 1e-6
PIVOT_MARGIN = 1e-9


# ======================================================================================================================
# reference

def default_cam5(H, W):
    """batch.py:111's calibration scaled to an H x W image, and the baseline: fx, fy, cx, cy, b."""
    fx, fy, cx, cy = T.CAM[:4]
    return np.array([fx * W / 1920.0, fy * H / 1080.0, cx * W / 1920.0, cy * H / 1080.0, BASELINE], np.float64)


class Margins:
    """The smallest distance of any decision from its bound, over everything one call decided."""

    def __init__(self):
        self.inlier = np.inf       # min |e2 / (thr2 Xz^2) - 1| and, for points near the camera plane, |Xz| / |P - t|
        self.degenerate = np.inf   # min |n3 / (1e-6 n1 n2) - 1|
        self.pivot = np.inf        # min |d| / H[j][j] over the Cholesky pivots d

    def safe(self):
        return self.inlier > MARGIN and self.degenerate > MARGIN and self.pivot > PIVOT_MARGIN

    def __repr__(self):
        return f"Margins(inlier={self.inlier:.3g}, degenerate={self.degenerate:.3g}, pivot={self.pivot:.3g})"


def points(x, y, d, cam):
    fx, fy, cx, cy, b = (np.float64(v) for v in cam[:5])
    fb = fx * b
    Z = fb / d
    return np.stack([((x - cx) * Z) / fx, ((y - cy) * Z) / fy, Z], -1)


def triad(A, B, C, mg=None):
    """(e [3,3] rows e1 e2 e3, ok)."""
    e1, f = B - A, C - A
    c3 = np.array([e1[1] * f[2] - e1[2] * f[1], e1[2] * f[0] - e1[0] * f[2], e1[0] * f[1] - e1[1] * f[0]])
    n1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
    n2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]
    n3 = (c3[0] * c3[0] + c3[1] * c3[1]) + c3[2] * c3[2]
    bound = np.float64(1e-6) * (n1 * n2)
    if mg is not None and not (n3 == 0 and bound == 0):           # 0 > 0 is false in any arithmetic
        mg.degenerate = min(mg.degenerate, abs(n3 / bound - 1.0) if bound > 0 else np.inf)
    if not (n3 > bound):
        return None, False
    e1 = e1 / np.sqrt(n1)
    e3 = c3 / np.sqrt(n3)
    e2 = np.array([e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]])
    return np.stack([e1, e2, e3]), True


def sample(h, k, n):
    r1, r2, r3 = mix(h ^ (3 * k)), mix(h ^ (3 * k + 1)), mix(h ^ (3 * k + 2))
    i = r1 % n
    j = (i + 1 + r2 % (n - 1)) % n
    l = r3 % (n - 2)
    if l >= min(i, j):
        l += 1
    if l >= max(i, j):
        l += 1
    return i, j, l


def model(P, Q, ijl, mg=None):
    """flat12 of the hypothesis with sample (i, j, l), or None."""
    i, j, l = ijl
    F, okp = triad(P[i], P[j], P[l], mg)
    E, okq = triad(Q[i], Q[j], Q[l], mg)
    if not (okp and okq):
        return None
    R = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            R[r, c] = (F[0, r] * E[0, c] + F[1, r] * E[1, c]) + F[2, r] * E[2, c]
    t = np.array([P[i, r] - ((R[r, 0] * Q[i, 0] + R[r, 1] * Q[i, 1]) + R[r, 2] * Q[i, 2]) for r in range(3)])
    return np.concatenate([R.reshape(-1), t])


def transform(T12, P):
    """X = R^T (P - t), [n,3]."""
    D = P - T12[9:]
    return np.stack([(T12[c] * D[:, 0] + T12[3 + c] * D[:, 1]) + T12[6 + c] * D[:, 2] for c in range(3)], 1)


def inliers(T12, P, u, v, cam, thr2, mg=None):
    fx, fy, cx, cy = (np.float64(w) for w in cam[:4])
    X = transform(T12, P)
    ex = fx * X[:, 0] - (u - cx) * X[:, 2]
    ey = fy * X[:, 1] - (v - cy) * X[:, 2]
    e2, lim = ex * ex + ey * ey, thr2 * (X[:, 2] * X[:, 2])
    if mg is not None and len(P):
        with np.errstate(all="ignore"):
            front = X[:, 2] > 0
            m = np.abs(e2[front] / lim[front] - 1.0)
            mz = np.abs(X[:, 2]) / np.maximum(np.linalg.norm(P - T12[9:], axis=1), 1e-300)
            mg.inlier = min([mg.inlier, float(mz.min())] + ([float(m.min())] if len(m) else []))
    return (X[:, 2] > 0) & (e2 <= lim), X


def jacobians(X, u, v, cam):
    """(r [n,2], J [n,2,6]) of the header's refit statement."""
    fx, fy, cx, cy = (np.float64(w) for w in cam[:4])
    iz = 1.0 / X[:, 2]
    a, b, px, py = fx * iz, fy * iz, X[:, 0] * iz, X[:, 1] * iz
    r = np.stack([(fx * px + cx) - u, (fy * py + cy) - v], 1)
    g2, h2 = -(a * px), -(b * py)
    z = np.zeros_like(a)
    J0 = np.stack([-(g2 * X[:, 1]), g2 * X[:, 0] - a * X[:, 2], a * X[:, 1], -a, z, -g2], 1)
    J1 = np.stack([b * X[:, 2] - h2 * X[:, 1], h2 * X[:, 0], -(b * X[:, 0]), z, -b, -h2], 1)
    return r, np.stack([J0, J1], 1)


def normal_equations(X, u, v, cam):
    r, J = jacobians(X, u, v, cam)
    H = np.einsum("nkp,nkq->pq", J, J)
    g = np.einsum("nkp,nk->p", J, r)
    return H, g, float((r * r).sum())


def cholesky_solve(H, g, mg=None):
    """H^-1 g, or None at a pivot that is not > 0 (the header's order of operations)."""
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - (L[j, :j] * L[j, :j]).sum()
        if mg is not None and H[j, j] > 0:
            mg.pivot = min(mg.pivot, abs(d / H[j, j]))
        if not (d > 0):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (g[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def retract(T12, xi):
    """T Exp(xi), xi = (omega, v): gtsam's Pose3::Expmap, as se3_device.h's pose_retract."""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th2 = float(w @ w)
    Wx = hat(w)
    if th2 <= 2.220446049250313e-16:
        Re, b, c = np.eye(3) + Wx, 0.5, 1.0 / 6.0
    else:
        th = np.sqrt(th2)
        sh = np.sin(0.5 * th)
        b = 2.0 * sh * sh / th2
        c = (th - np.sin(th)) / (th2 * th)
        Re = np.eye(3) + (np.sin(th) / th) * Wx + b * (Wx @ Wx)
    te = v + b * np.cross(w, v) + c * np.cross(w, np.cross(w, v))
    R = T12[:9].reshape(3, 3)
    return np.concatenate([(R @ Re).reshape(-1), T12[9:] + R @ te])


IDENTITY12 = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def pair_pose(x1, y1, d1, x2, y2, d2, cam, threshold_px, n_hyp, seed, c, refine_iters, mg=None):
    """One pair: its candidates as float64 arrays in index order (integers in the kernel; any real here).  Returns
    dict(T [12], JtJ [6,6], rss, keep [n] bool, info (6 ints), counts [n_hyp])."""
    x1, y1, d1, x2, y2, d2 = (np.asarray(a, np.float64) for a in (x1, y1, d1, x2, y2, d2))
    cam = np.asarray(cam, np.float64)
    thr2 = np.float64(threshold_px) * np.float64(threshold_px)
    n = len(x1)
    out = dict(T=IDENTITY12.copy(), JtJ=np.zeros((6, 6)), rss=0.0, keep=np.zeros(n, bool), counts=np.zeros(0, np.int64))
    if n < 3:
        out["info"] = (n, -1, -1, 0, 1, 0)
        return out
    P, Q, u, v = points(x1, y1, d1, cam), points(x2, y2, d2, cam), x2, y2
    h = mix(seed + 0x9E3779B9 * (c + 1))
    counts, best, best_count = [], -1, -1
    for k in range(n_hyp):
        Tk = model(P, Q, sample(h, k, n), mg)
        cnt = -1 if Tk is None else int(inliers(Tk, P, u, v, cam, thr2, mg)[0].sum())
        counts.append(cnt)
        if cnt > best_count:                               # strict: the lowest k wins a tie
            best, best_count = k, cnt
    out["counts"] = np.array(counts, np.int64)
    if best < 0:
        out["info"] = (n, -1, -1, 0, 2, 0)
        return out
    Tc = model(P, Q, sample(h, best, n))
    status, rounds = 0, 0
    for it in range(refine_iters + 1):
        inl, X = inliers(Tc, P, u, v, cam, thr2, mg)
        H, g, rss = normal_equations(X[inl], u[inl], v[inl], cam)
        if it == refine_iters:
            break
        delta = cholesky_solve(H, g, mg) if inl.sum() >= 3 else None
        if delta is None:
            status = 3
            break
        Tc = retract(Tc, -delta)
        rounds += 1
    out["T"] = Tc
    if status == 0:
        out.update(JtJ=H, rss=rss, keep=inl)
    out["info"] = (n, best, best_count, int(inl.sum()) if status == 0 else 0, status, rounds)
    return out


def candidates(t, c):
    """Slots and per-candidate integers of pair c of a table dict: (src, dst, x1, y1, d1, x2, y2, d2); src empty for a
    refused pair."""
    K, W, Fn = t["match_idx"].shape[1], t["W"], len(t["stereo_idx"])
    a, b = int(t["pair_a"][c]), int(t["pair_b"][c])
    empty = (np.zeros(0, np.int64),) * 8
    if not (0 <= a < Fn and 0 <= b < Fn and a != b):
        return empty
    cnt = [T._clamp_count(t["kp_count"][q], K) for q in (2 * a, 2 * a + 1, 2 * b, 2 * b + 1)]
    nla, nra, nlb, nrb = cnt
    i = np.arange(nla)
    j = t["match_idx"][c, :nla].astype(np.int64)
    ok = (j >= 0) & (j < nlb)
    i, j = i[ok], j[ok]
    sa, sb = t["stereo_idx"][a, i].astype(np.int64), t["stereo_idx"][b, j].astype(np.int64)
    ok = (sa >= 0) & (sa < nra) & (sb >= 0) & (sb < nrb)
    i, j, sa, sb = i[ok], j[ok], sa[ok], sb[ok]
    x1, y1 = decode(t["kp_keys"][2 * a, i], W)
    xr1, _ = decode(t["kp_keys"][2 * a + 1, sa], W)
    x2, y2 = decode(t["kp_keys"][2 * b, j], W)
    xr2, _ = decode(t["kp_keys"][2 * b + 1, sb], W)
    d1, d2 = x1 - xr1, x2 - xr2
    ok = (d1 >= 1) & (d2 >= 1)
    return i[ok], j[ok], x1[ok], y1[ok], d1[ok], x2[ok], y2[ok], d2[ok]


def stereo_pair_pose(t, threshold_px, n_hyp, seed, refine_iters, mg=None):
    """vus_stereo_pair_pose on a table dict: dict(T_ab [P,12], JtJ [P,36], rss [P], match_idx_out [P,K], info [P,6])."""
    Pn, K = t["match_idx"].shape
    res = dict(T_ab=np.zeros((Pn, 12)), JtJ=np.zeros((Pn, 36)), rss=np.zeros(Pn), match_idx_out=np.full((Pn, K), -1, np.int32),
               info=np.zeros((Pn, 6), np.int32))
    for c in range(Pn):
        src, dst, *cand = candidates(t, c)
        o = pair_pose(*cand, t["cam"], threshold_px, n_hyp, seed, c, refine_iters, mg)
        res["T_ab"][c], res["JtJ"][c], res["rss"][c], res["info"][c] = o["T"], o["JtJ"].reshape(-1), o["rss"], o["info"]
        res["match_idx_out"][c, src[o["keep"]]] = dst[o["keep"]]
    return res


# ======================================================================================================================
# generators

def pose12(w, t):
    return np.concatenate([rodrigues(w).reshape(-1), np.asarray(t, np.float64)])


def pose_error(T12, truth12):
    """(translation error in metres, rotation error in radians)."""
    dR = T12[:9].reshape(3, 3).T @ truth12[:9].reshape(3, 3)
    v = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])     # 2 sin(angle) axis: exact near zero
    return (float(np.linalg.norm(T12[9:] - truth12[9:])),
            float(np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(dR) - 1.0))))


def planted_pair(rng, n_true, n_wrong, T12, H, W, cam=None, zrange=(2.5, 4.2), quantise=True):
    """Candidates of one pair with P_a = R Q_b + t planted: points zrange metres in front of camera a, projected into both
    rigs.  quantise: pixel positions and right-image columns rounded to integers (the disparity is their difference);
    otherwise exact reals.  Wrong matches pair a true left(a) observation with an unrelated one of left(b).  Returns
    (x1, y1, d1, x2, y2, d2, truth [n] bool), shuffled."""
    cam = default_cam5(H, W) if cam is None else cam
    fx, fy, cx, cy, b = cam
    R, t = T12[:9].reshape(3, 3), T12[9:]

    def observe(p):
        z = p[2]
        if z <= 0.5:
            return None
        x, y, d = p[0] / z * fx + cx, p[1] / z * fy + cy, fx * b / z
        if quantise:
            xr = round(x - d)
            x, y = round(x), round(y)
            d = x - xr
        if not (BORDER + 40 <= x < W - BORDER and BORDER <= y < H - BORDER and d >= 1):
            return None                      # 40 px: room for the right-image column left of x
        return x, y, d

    def draw():
        while True:
            z = rng.uniform(*zrange)
            pa = np.array([(rng.uniform(0, W) - cx) / fx * z, (rng.uniform(0, H) - cy) / fy * z, z])
            oa, ob = observe(pa), observe(R.T @ (pa - t))
            if oa is not None and ob is not None:
                return oa, ob

    rows = [sum(draw(), ()) for _ in range(n_true)]
    for _ in range(n_wrong):
        rows.append(draw()[0] + draw()[1])
    rows = np.array(rows, np.float64).reshape(-1, 6)
    perm = rng.permutation(len(rows))
    rows = rows[perm]
    return tuple(rows[:, q] for q in range(6)) + (perm < n_true,)


def tables_from_pairs(rng, pairs, F, K, H, W):
    """Tables of F frames whose pair c = pairs[c] = (a, b, (x1, y1, d1, x2, y2, d2, ...)) holds those candidates at random
    slots.  Every (pair, side) takes its own slots of its frame's left and right lists, so a frame may serve several
    pairs; every other slot holds a random key and no match.  dict(match_idx [P,K], pair_a, pair_b, stereo_idx [F,K],
    kp_keys [2F,K], kp_count [2F], H, W, src [P] slots of the candidates in the order given)."""
    Pn = len(pairs)
    keys = ((rng.integers(0, 256, (2 * F, K)).astype(np.uint32) << 24) | rng.integers(0, H * W, (2 * F, K)).astype(np.uint32))
    stereo = np.full((F, K), -1, np.int32)
    match = np.full((Pn, K), -1, np.int32)
    perm = [rng.permutation(K) for _ in range(2 * F)]
    used = [0] * (2 * F)

    def take(img, n):
        assert used[img] + n <= K, (img, used[img], n, K)
        s = perm[img][used[img]:used[img] + n]
        used[img] += n
        return s

    def place(f, x, y, d):
        n = len(x)
        sl, sr = take(2 * f, n), take(2 * f + 1, n)
        x, y, d = (np.asarray(q).astype(np.int64) for q in (x, y, d))
        assert ((x - d >= 0) & (x - d < W) & (x >= 0) & (x < W) & (y >= 0) & (y < H)).all()
        score = rng.integers(0, 256, n).astype(np.uint32) << 24
        keys[2 * f, sl] = score | (y * W + x).astype(np.uint32)
        keys[2 * f + 1, sr] = score | (y * W + (x - d)).astype(np.uint32)
        stereo[f, sl] = sr
        return sl

    src = []
    for c, (a, b, m) in enumerate(pairs):
        sa, sb = place(a, m[0], m[1], m[2]), place(b, m[3], m[4], m[5])
        match[c, sa] = sb
        src.append(sa)
    return dict(match_idx=match, pair_a=np.array([p[0] for p in pairs], np.int32), pair_b=np.array([p[1] for p in pairs], np.int32),
                stereo_idx=stereo, kp_keys=keys, kp_count=np.full(2 * F, K, np.int32), H=H, W=W, src=src)


PLANTED_H, PLANTED_W, THRESHOLD = 720, 1280, 2.0
# the planted revisit of the accuracy test: 0.3 m apart, some yaw and tilt
PLANTED_POSE = pose12((0.03, -0.05, 0.35), (0.3, -0.05, 0.04))
# Quantised planted fixture: 300 true + 150 wrong matches at 1280 x 720, 18-31 px of disparity (2.5-4.2 m).  The bounds
# are twice the largest error this reference makes over the eight pairs of test_loop_ref's quantised test -- 12.8 mm and
# 3.70e-3 rad, measured with this file (profiles/loop_closure.md) -- a statement about integer disparities, not the kernel.
QUANTISED = dict(n_true=300, n_wrong=150, n_pairs=8, seed=41, n_hyp=256, refine_iters=10,
                 bound_t_m=2 * 0.0128, bound_r_rad=2 * 0.00370)


def planted_tables(seed, K, sizes, frames=None, H=PLANTED_H, W=PLANTED_W, zrange=(2.5, 4.2)):
    """A batch whose pair c is a planted scene of sizes[c] = (n_true, n_wrong) with its own pose; frames[c] = (a, b),
    default (2c, 2c+1)."""
    rng = np.random.default_rng(seed)
    frames = [(2 * c, 2 * c + 1) for c in range(len(sizes))] if frames is None else frames
    pairs, truth = [], []
    for (n_true, n_wrong), (a, b) in zip(sizes, frames):
        T12 = pose12(rng.normal(size=3) * 0.15, rng.normal(size=3) * 0.15)
        pairs.append((a, b, planted_pair(rng, n_true, n_wrong, T12, H, W, zrange=zrange)))
        truth.append(T12)
    t = tables_from_pairs(rng, pairs, 1 + max(max(f) for f in frames), K, H, W)
    t["truth"] = np.array(truth)
    return t


def _explicit(rng, rows):
    """A candidate tuple from (x1, y1, d1, x2, y2, d2) rows."""
    r = np.array(rows, np.float64).reshape(-1, 6)
    return tuple(r[:, q] for q in range(6))


def _adversarial(name):
    H, W = 480, 640
    if name == "few":
        # n = 0, 1, 2, 3 (n - 2 = 1), 4, then 3 and 4 again with wrong matches only
        rng = np.random.default_rng(51)
        Tp = pose12((0.0, 0.02, 0.1), (0.2, 0.0, 0.0))
        sizes = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, 3), (0, 4)]
        pairs = [(2 * c, 2 * c + 1, planted_pair(rng, nt, nw, Tp, H, W, zrange=(1.5, 2.5))) for c, (nt, nw) in enumerate(sizes)]
        return tables_from_pairs(rng, pairs, 2 * len(sizes), 40, H, W)
    if name == "collinear":
        # every candidate on one image row at one disparity: P and Q on a line, every sample degenerate (status 2)
        rng = np.random.default_rng(52)
        rows = [(100 + 9 * q, 200, 24, 90 + 9 * q, 200, 24) for q in range(40)]
        same = [(300, 240, 20, 310, 240, 20)] * 12                  # twelve copies of one point: n1 = n2 = n3 = 0
        return tables_from_pairs(rng, [(0, 1, _explicit(rng, rows)), (1, 2, _explicit(rng, same))], 3, 64, H, W)
    if name == "no_disparity":
        # disparities 0 and negative on either side: no candidates; pair 2 mixes 5 good ones in
        rng = np.random.default_rng(53)
        Tp = pose12((0.0, 0.0, 0.05), (0.1, 0.0, 0.0))
        g = planted_pair(rng, 30, 0, Tp, H, W, zrange=(1.5, 2.5))
        zero = tuple(np.where(np.arange(30) % 2 == 0, 0.0, -3.0) if q == 2 else g[q] for q in range(6))
        zero_b = tuple(np.where(np.arange(30) % 3 == 0, -1.0, 0.0) if q == 5 else g[q] for q in range(6))
        mixed = tuple(np.where(np.arange(30) < 25, 0.0, g[2]) if q == 2 else g[q] for q in range(6))
        return tables_from_pairs(rng, [(0, 1, zero), (2, 3, zero_b), (4, 5, mixed)], 6, 64, H, W)
    if name == "identical":
        # the same frame content on both sides: P = Q, the identity, zero residuals up to rounding
        rng = np.random.default_rng(54)
        pairs = []
        for c, n in enumerate((60, 3, 200)):
            g = planted_pair(rng, n, 0, IDENTITY12, H, W, zrange=(1.5, 2.5))
            pairs.append((2 * c, 2 * c + 1, g[:3] + g[:3]))
        return tables_from_pairs(rng, pairs, 6, 256, H, W)
    if name == "pairing":
        # a > b, a frame used by several pairs, a == b, frame numbers out of range on either side
        rng = np.random.default_rng(55)
        Tp = [pose12(rng.normal(size=3) * 0.1, rng.normal(size=3) * 0.1) for _ in range(7)]
        fr = [(3, 0), (0, 1), (0, 2), (2, 2), (1, 4), (-1, 2), (2, 0)]
        pairs = [(a, b, planted_pair(rng, 30, 10, Tp[c], H, W, zrange=(1.5, 2.5))) for c, (a, b) in enumerate(fr[:3] + fr[6:])]
        t = tables_from_pairs(rng, pairs, 4, 256, H, W)
        # the refused pairs get rows that WOULD be candidates of some frame if their numbers were taken at face value
        order = [0, 1, 2, None, None, None, 3]
        match = np.stack([t["match_idx"][q] if q is not None else t["match_idx"][1] for q in order])
        t.update(match_idx=match, pair_a=np.array([f[0] for f in fr], np.int32), pair_b=np.array([f[1] for f in fr], np.int32))
        return t
    if name == "bad_tables":
        # counts above K and negative, match and stereo indices out of range (below -1, at and above the count, huge)
        rng = np.random.default_rng(56)
        K = 200
        Tp = pose12((0.02, 0.0, 0.1), (0.15, 0.05, 0.0))
        fr = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (1, 2)]
        pairs = [(a, b, planted_pair(rng, 50, 20, Tp, H, W, zrange=(1.5, 2.5))) for a, b in fr]
        t = tables_from_pairs(rng, pairs, 10, K, H, W)
        cnt = t["kp_count"]
        cnt[0], cnt[3] = K + 57, 2 ** 30                    # oversize: clamped to K
        cnt[4] = -5                                         # left(2) empty: pair 1 has no candidates
        cnt[11] = -1                                        # right(5) empty: pair 2 has no candidates
        cnt[12], cnt[14], cnt[15] = 120, 90, 100            # counts that cut live slots off (pair 3)
        cnt[17] = 0                                         # right(8) empty
        for tab, hi in ((t["match_idx"], K), (t["stereo_idx"], K)):
            live = np.argwhere(tab >= 0)
            pick = live[rng.random(len(live)) < 0.15]
            bad = rng.choice(np.array([-2, -1000, hi, hi + 1, 2 ** 31 - 1, -2 ** 31], np.int64), len(pick))
            tab[pick[:, 0], pick[:, 1]] = bad.astype(np.int32)
            dead = np.argwhere(tab < 0)
            pick = dead[rng.random(len(dead)) < 0.1]
            tab[pick[:, 0], pick[:, 1]] = rng.integers(0, hi, len(pick)).astype(np.int32)     # stray matches of random keys
        return t
    raise KeyError(name)


ADVERSARIAL = ("few", "collinear", "no_disparity", "identical", "pairing", "bad_tables")

# planted batches for the kernel test, by max_kp.  1: a single slot per image (n <= 1); 65 and 257: one past a wave and one
# past the block in the compaction; 2000: the timing shape; 4096: the LDS maximum, every slot a candidate in pair 0
PLANTED_KP = {
    1: dict(seed=61, K=1, sizes=[(1, 0), (0, 1)]),
    64: dict(seed=62, K=64, sizes=[(40, 20), (20, 44), (64, 0)]),
    65: dict(seed=63, K=65, sizes=[(45, 20), (5, 40)]),
    257: dict(seed=64, K=257, sizes=[(200, 57), (100, 100)]),
    2000: dict(seed=65, K=2000, sizes=[(300, 150), (1200, 800), (40, 24)]),
    4096: dict(seed=66, K=4096, sizes=[(2600, 1496), (300, 150)]),
}
# nine pairs, nine poses, different sizes: indexing the hash, the outputs or info by the wrong pair shows
BATCH9 = dict(seed=67, K=128, sizes=[(40 + 5 * c, 30 - 3 * c) for c in range(9)])

N_HYP, SEED, REFINE = 64, 20261019, 10
_cache = {}


def tables(name):
    if ("tables", name) not in _cache:
        if name in ADVERSARIAL:
            t = _adversarial(name)
        elif name == "batch9":
            t = planted_tables(**BATCH9)
        else:
            t = planted_tables(**PLANTED_KP[int(name.removeprefix("planted_kp"))])
        t["cam"] = default_cam5(t["H"], t["W"])
        _cache["tables", name] = t
    return _cache["tables", name]


def case(name, threshold_px=THRESHOLD, n_hyp=N_HYP, seed=SEED, refine_iters=REFINE):
    """(tables incl. cam, the reference's outputs), built once per session and certified margin-safe: the kernel may then
    differ from the reference by rounding only."""
    key = (name, threshold_px, n_hyp, seed, refine_iters)
    if key not in _cache:
        t = tables(name)
        mg = Margins()
        ref = stereo_pair_pose(t, threshold_px, n_hyp, seed, refine_iters, mg)
        assert mg.safe(), (key, mg)
        _cache[key] = (t, ref)
    return _cache[key]
