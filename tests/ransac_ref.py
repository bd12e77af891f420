"""Plain numpy statement of vus_two_point_ransac (include/vus_ransac.h) and the generators of the match tables it is
tested on.  Test infrastructure only (a plain module, not a conftest).

The reference half restates the header operation by operation: float64 arrays combined with + - * / in the header's
order (numpy does not contract a multiply and an add), the hash in Python integers, vectorised over the matches of a
pair with a plain loop over the hypotheses.  Positions are decoded and counts clamped as tests/track_ref.py does for
vus_track_ids.  The kernel (built without FMA contraction) must agree with it bit for bit.

The generator half builds (a) planted scenes: a rotation, a translation, points 2-6 m in front of the first camera,
projected into both frames, rounded to integer pixels inside the 31-px border, with uniformly random wrong pairs
shuffled in; (b) adversarial tables in the style of track_ref.make_tables.
"""
import numpy as np

import track_ref as T

M32 = 0xFFFFFFFF
BORDER = 31


# ======================================================================================================================
# reference

def mix(v):
    """lowbias32 (synth._mix32) on a Python int."""
    v &= M32
    v ^= v >> 16
    v = (v * 0x7FEB352D) & M32
    v ^= v >> 15
    v = (v * 0x846CA68B) & M32
    v ^= v >> 16
    return v


def default_cam(H, W):
    """batch.py:111's calibration (given for 1920 x 1080) scaled to an H x W image: fx, fy, cx, cy."""
    fx, fy, cx, cy = T.CAM[:4]
    return np.array([fx * W / 1920.0, fy * H / 1080.0, cx * W / 1920.0, cy * H / 1080.0], np.float64)


def thresholds(cam, threshold_px):
    fx, fy = np.float64(cam[0]), np.float64(cam[1])
    tn = np.float64(threshold_px) / ((fx + fy) / np.float64(2.0))
    return tn * tn


def pair_ransac(x1, y1, x2, y2, R9, cam, threshold_px, n_hyp, seed, p):
    """One frame pair: matches as float64 pixel arrays in index order.  Returns (keep [n] bool, best, n_static,
    counts [n_hyp] (the count_k of every hypothesis; empty if n < 2))."""
    x1, y1, x2, y2 = (np.asarray(v, np.float64) for v in (x1, y1, x2, y2))
    r = np.asarray(R9, np.float64).reshape(9)
    fx, fy, cx, cy = (np.float64(v) for v in np.asarray(cam, np.float64)[:4])
    tn2 = thresholds(cam, threshold_px)
    n = len(x1)
    with np.errstate(all="ignore"):
        a1, b1, a2, b2 = (x1 - cx) / fx, (y1 - cy) / fy, (x2 - cx) / fx, (y2 - cy) / fy
        X = (r[0] * a1 + r[1] * b1) + r[2]
        Y = (r[3] * a1 + r[4] * b1) + r[5]
        Z = (r[6] * a1 + r[7] * b1) + r[8]
        front = Z > 0
        dx, dy = a2 * Z - X, b2 * Z - Y
        static = front & ((dx * dx + dy * dy) <= tn2 * (Z * Z))
        mx, my, mz = Y - Z * b2, Z * a2 - X, X * b2 - Y * a2
        counts = []
        best, best_count, best_inl = -1, -1, None
        if n >= 2:
            a = mix(seed + 0x9E3779B9 * (p + 1))
            for k in range(n_hyp):
                r1, r2 = mix(a ^ (2 * k)), mix(a ^ (2 * k + 1))
                i = r1 % n
                j = (i + 1 + r2 % (n - 1)) % n
                tx = my[i] * mz[j] - mz[i] * my[j]
                ty = mz[i] * mx[j] - mx[i] * mz[j]
                tz = mx[i] * my[j] - my[i] * mx[j]
                lx, ly, lz = ty * Z - tz * Y, tz * X - tx * Z, tx * Y - ty * X
                e = (lx * a2 + ly * b2) + lz
                q = lx * lx + ly * ly
                inl = front & (static | ((q > 0) & (e * e <= tn2 * q)))
                c = int(inl.sum()) if front[i] and front[j] else -1
                counts.append(c)
                if c > best_count:                     # strict: the lowest k wins a tie
                    best, best_count, best_inl = k, c, inl
    keep = front.copy() if best < 0 else best_inl
    return keep, best, int(static.sum()), np.array(counts, np.int64)


def decode(keys, W):
    pos = np.asarray(keys).astype(np.int64) & T.POS_MASK
    return (pos % W).astype(np.float64), (pos // W).astype(np.float64)


def two_point_ransac(track_idx, kp_keys, kp_count, H, W, rot, cam, threshold_px, n_hyp, seed):
    """vus_two_point_ransac: (track_idx_out [F-1,K] int32, info [F-1,4] int32)."""
    track_idx = np.asarray(track_idx)
    P, K = track_idx.shape
    out = np.full((P, K), -1, np.int32)
    info = np.zeros((P, 4), np.int32)
    for p in range(P):
        nl, nn = T._clamp_count(kp_count[2 * p], K), T._clamp_count(kp_count[2 * p + 2], K)
        t = track_idx[p, :nl].astype(np.int64)
        src = np.nonzero((t >= 0) & (t < nn))[0]
        dst = t[src]
        x1, y1 = decode(kp_keys[2 * p, src], W)
        x2, y2 = decode(kp_keys[2 * p + 2, dst], W)
        keep, best, n_static, _ = pair_ransac(x1, y1, x2, y2, rot[p], cam, threshold_px, n_hyp, seed, p)
        out[p, src[keep]] = dst[keep]
        info[p] = (len(src), int(keep.sum()), best, n_static)
    return out, info


# ======================================================================================================================
# generators

def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def planted_pair(rng, n_true, n_wrong, t, w, H, W, cam=None):
    """Matches of one frame pair with the camera motion p2 = R p1 + t, R = exp(w) (= R_cur_prev).  Returns
    (x1, y1, x2, y2 int64 [n], truth [n] bool, R9), true and wrong matches shuffled."""
    cam = default_cam(H, W) if cam is None else cam
    fx, fy, cx, cy = cam
    R, t = rodrigues(w), np.asarray(t, np.float64)
    rows = []
    while len(rows) < n_true:
        x, y, z = rng.uniform(BORDER, W - BORDER), rng.uniform(BORDER, H - BORDER), rng.uniform(2.0, 6.0)
        p2 = R @ np.array([(x - cx) / fx * z, (y - cy) / fy * z, z]) + t
        if p2[2] <= 0:
            continue
        u, v = p2[0] / p2[2] * fx + cx, p2[1] / p2[2] * fy + cy
        if BORDER <= u < W - BORDER and BORDER <= v < H - BORDER:
            rows.append((round(x), round(y), round(u), round(v)))
    true = np.array(rows, np.int64).reshape(-1, 4)
    wrong = np.stack([rng.integers(BORDER, W - BORDER, n_wrong), rng.integers(BORDER, H - BORDER, n_wrong),
                      rng.integers(BORDER, W - BORDER, n_wrong), rng.integers(BORDER, H - BORDER, n_wrong)], 1)
    allm = np.concatenate([true, wrong.astype(np.int64)])
    perm = rng.permutation(len(allm))
    allm = allm[perm]
    return allm[:, 0], allm[:, 1], allm[:, 2], allm[:, 3], perm < n_true, R.reshape(-1)


def tables_from_pairs(rng, pairs, K, H, W, overlap=False):
    """Match tables of len(pairs) + 1 frames whose pair p holds the matches pairs[p] = (x1, y1, x2, y2, ...) at random
    slots: dict(track_idx [P,K], kp_keys [2(P+1),K], kp_count, H, W, src [P] (the slot of every match, in the order
    given)).  Every other slot holds a random key and no match.  overlap=False: a left image keeps the targets of the
    previous pair and the sources of its own pair in disjoint slots (needs K >= both together).  overlap=True: the two
    slot sets are drawn independently; where they collide the source's position stands (the earlier pair's match then
    points at some other pixel: still a table, no longer the planted one)."""
    P = len(pairs)
    F = P + 1
    keys = ((rng.integers(0, 256, (2 * F, K)).astype(np.uint32) << 24) | rng.integers(0, H * W, (2 * F, K)).astype(np.uint32))
    track = np.full((P, K), -1, np.int32)
    src_slots, dst_slots = [], []
    for f in range(F):
        nA = len(pairs[f - 1][0]) if f > 0 else 0
        nB = len(pairs[f][0]) if f < P else 0
        if overlap:
            sA, sB = rng.permutation(K)[:nA], rng.permutation(K)[:nB]
        else:
            assert nA + nB <= K, (nA, nB, K)
            perm = rng.permutation(K)
            sA, sB = perm[:nA], perm[nA:nA + nB]
        score = rng.integers(0, 256, K).astype(np.uint32) << 24
        if nA:
            keys[2 * f, sA] = score[sA] | (pairs[f - 1][3] * W + pairs[f - 1][2]).astype(np.uint32)
        if nB:
            keys[2 * f, sB] = score[sB] | (pairs[f][1] * W + pairs[f][0]).astype(np.uint32)
        dst_slots.append(sA)
        src_slots.append(sB)
    for p in range(P):
        track[p, src_slots[p]] = dst_slots[p + 1]
    return dict(track_idx=track, kp_keys=keys, kp_count=np.full(2 * F, K, np.int32), H=H, W=W, src=src_slots[:P])


def small_rotations(rng, P, scale=0.05):
    return np.stack([rodrigues(rng.normal(size=3) * scale).reshape(-1) for _ in range(P)])


# the planted cases of the issue: (true, wrong, n_hyp, t, w)
GENERAL_T, GENERAL_W = (0.1, 0.2, 0.05), (0.02, -0.03, 0.05)
PLANTED = {
    "sideways_yaw": (300, 100, 128, (0.25, 0.0, 0.0), (0.0, 0.0, 0.05)),
    "general": (300, 300, 128, GENERAL_T, GENERAL_W),
    "pure_translation": (40, 24, 64, (0.0, 0.25, 0.0), (0.0, 0.0, 0.0)),
    "pure_rotation": (300, 300, 128, (0.0, 0.0, 0.0), (0.01, 0.02, 0.03)),
    "general_large": (600, 600, 256, GENERAL_T, GENERAL_W),
}
PLANTED_H, PLANTED_W, PLANTED_THRESHOLD = 720, 1280, 3.0


def planted_tables(seed, K, sizes, H=PLANTED_H, W=PLANTED_W, overlap=False):
    """A batch whose pair p is a planted scene of sizes[p] = (n_true, n_wrong) with its own motion."""
    rng = np.random.default_rng(seed)
    pairs, rot = [], []
    for n_true, n_wrong in sizes:
        t = rng.normal(size=3) * 0.15
        w = rng.normal(size=3) * 0.04
        pr = planted_pair(rng, n_true, n_wrong, t, w, H, W)
        pairs.append(pr)
        rot.append(pr[5])
    tb = tables_from_pairs(rng, pairs, K, H, W, overlap=overlap)
    tb["rot"] = np.array(rot, np.float64).reshape(-1, 9)
    return tb


def rot_y(th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _adversarial(name):
    """dict(track_idx, kp_keys, kp_count, H, W, rot) of one adversarial case."""
    H, W = 480, 640
    if name == "make_tables":
        # colliding targets, indices out of range on both sides, counts above K (images 0 and 6), a negative count (image
        # 8: the left image of frame 4 -- pair 3 has no target, pair 4 no source), an empty left list (frame 6)
        t = T.make_tables(21, F=9, K=200, H=H, W=W, over=(0, 6), negative=(8,), no_left=(6,), p_collide=0.2, p_oob=0.1)
        t["rot"] = small_rotations(np.random.default_rng(22), 8)
        return t
    if name == "few_matches":
        # pair p has n = p matches for p = 0..3, then 2 and 3 again with wrong pairs only
        rng = np.random.default_rng(23)
        pairs = [planted_pair(rng, n, 0, (0.2, 0.0, 0.0), (0, 0, 0.02), H, W) for n in (0, 1, 2, 3)]
        pairs += [planted_pair(rng, 0, n, (0.2, 0.0, 0.0), (0, 0, 0.02), H, W) for n in (2, 3)]
        t = tables_from_pairs(rng, pairs, 40, H, W)
        t["rot"] = np.array([pr[5] for pr in pairs]).reshape(-1, 9)
        return t
    if name == "all_static_identity":
        # nothing moves and R = I: every m is exactly 0, every model t exactly 0 (q = 0), everything survives as `static`
        rng = np.random.default_rng(24)
        pairs = []
        for n in (50, 2, 150):
            x, y = rng.integers(BORDER, W - BORDER, n), rng.integers(BORDER, H - BORDER, n)
            pairs.append((x, y, x.copy(), y.copy()))
        t = tables_from_pairs(rng, pairs, 200, H, W)
        t["rot"] = np.tile(np.eye(3).reshape(-1), (3, 1))
        return t
    if name == "behind":
        # a turn of 80 degrees about y: rays right of the centre get Z <= 0 in the second camera -- not `front`: never
        # inliers, and a hypothesis that samples one counts -1; in pair 2 EVERY ray is behind (R = diag(1, -1, -1))
        rng = np.random.default_rng(25)
        pairs = [planted_pair(rng, 0, 120, (0, 0, 0), (0, 0, 0), H, W) for _ in range(3)]
        t = tables_from_pairs(rng, pairs, 250, H, W)
        t["rot"] = np.stack([rot_y(np.deg2rad(80.0)).reshape(-1), rot_y(np.deg2rad(-75.0)).reshape(-1),
                             np.diag([1.0, -1.0, -1.0]).reshape(-1)])
        return t
    if name == "all_outliers":
        rng = np.random.default_rng(26)
        pairs = [planted_pair(rng, 0, n, (0, 0, 0), (0, 0, 0), H, W) for n in (90, 17)]
        t = tables_from_pairs(rng, pairs, 128, H, W)
        t["rot"] = small_rotations(rng, 2)
        return t
    raise KeyError(name)


ADVERSARIAL = ("make_tables", "few_matches", "all_static_identity", "behind", "all_outliers")

# planted batches for the kernel test, by max_kp.  1: a single slot per image (n <= 1: no model); 64 and 2000: disjoint
# slots; 2000 holds the issue's case sizes side by side (1800 of 2000 slots used in the fullest image)
PLANTED_KP = {
    1: dict(seed=31, K=1, sizes=[(1, 0), (0, 1), (1, 0)], overlap=True),
    64: dict(seed=32, K=64, sizes=[(20, 10), (25, 5), (3, 27)]),
    2000: dict(seed=33, K=2000, sizes=[(300, 100), (300, 300), (40, 24), (300, 300), (600, 600)]),
}
# nine pairs, nine rotations, different sizes: indexing rot, the hash or info by the wrong pair shows
BATCH9 = dict(seed=34, K=128, sizes=[(30 + 3 * p, 20 - 2 * p) for p in range(9)])
# one pair of about 4000 matches in 8192 slots: beyond the matches whose values the kernel keeps in LDS
LARGE = dict(seed=35, K=8192, sizes=[(2600, 1400)])

_cache = {}


def case(name, threshold_px=PLANTED_THRESHOLD, n_hyp=64, seed=20261004):
    """(tables incl. rot and cam, (track_idx_out, info) of the reference), built once per session."""
    key = (name, threshold_px, n_hyp, seed)
    if key not in _cache:
        if ("tables", name) not in _cache:
            if name in ADVERSARIAL:
                t = _adversarial(name)
            elif name == "batch9":
                t = planted_tables(**BATCH9)
            elif name == "large":
                t = planted_tables(**LARGE)
            else:
                t = planted_tables(**PLANTED_KP[int(name.removeprefix("planted_kp"))])
            t["cam"] = default_cam(t["H"], t["W"])
            _cache["tables", name] = t
        t = _cache["tables", name]
        _cache[key] = (t, two_point_ransac(t["track_idx"], t["kp_keys"], t["kp_count"], t["H"], t["W"], t["rot"], t["cam"],
                                           threshold_px, n_hyp, seed))
    return _cache[key]
