"""Plain reference of the stages between the match tables and the factor graph, and the generator of the adversarial
tables they are tested on.  Test infrastructure only (a plain module, not a conftest).

The reference half restates, with dicts and loops as batch.py does, what the consumer of the CameraMeasurement stream
sees: the id propagation of the emitter (include/vus.h: vus_track_ids), `get_landmarks` (batch.py:144-176), the
landmark loop of `batch_create` (batch.py:295-305), the initial residual h(X, L) - z of GenericStereoFactor3D, the
mutual-match filter, the pyramid append and the initial-residual gate.  Floats are numpy float64 scalars combined
with + - * / in the order the header and batch.py:152-166 give, so the C oracle and the kernels (built without FMA
contraction) must agree with it bit for bit.

The generator half builds match tables from a seed with knobs for the densities of missing, stale, out-of-range and
colliding entries, and `*_properties` report, from the inputs and the REFERENCE's output alone, which of the edges a
case really contains: a test asserts them, so a generator that stops producing an edge fails instead of hiding it.
"""
import numpy as np

POS_MASK = 0x00FFFFFF
I32_MAX = 2 ** 31 - 1
I32_MIN = -2 ** 31


# ======================================================================================================================
# reference

def _clamp_count(c, max_kp):
    """Keypoints of an image that exist: the count, at most the list's capacity; a negative count is an empty list."""
    return max(0, min(int(c), max_kp))


def normalised(key, H, W):
    """(u, v) of a keypoint key in the message's convention: 2 x / W - 1, 2 y / H - 1."""
    pos = int(key) & POS_MASK
    x, y = pos % W, pos // W
    return (np.float64(2.0) * np.float64(x) / np.float64(W) - np.float64(1.0),
            np.float64(2.0) * np.float64(y) / np.float64(H) - np.float64(1.0))


def track_ids(stereo_idx, track_idx, kp_keys, kp_count, H, W):
    """The CameraMeasurement emitter.  Returns (ids [F,K] int64, feat [F,K,4] f64, n_ids, carried [F,K] int64) where
    carried[f, i] is the id the left keypoint i of frame f carries into frame f + 1, published or not (-1: none)."""
    stereo_idx = np.asarray(stereo_idx)
    F, K = stereo_idx.shape
    ids = np.full((F, K), -1, np.int64)
    feat = np.zeros((F, K, 4), np.float64)
    carried_out = np.full((F, K), -1, np.int64)
    carried = {}                      # left keypoint index of the previous frame -> id
    next_id = 0
    for f in range(F):
        nl, nr = _clamp_count(kp_count[2 * f], K), _clamp_count(kp_count[2 * f + 1], K)
        now = {}
        for ip in sorted(carried):    # the lowest-index predecessor THAT CARRIES AN ID claims its successor first
            j = int(track_idx[f - 1, ip])
            if 0 <= j < nl and j not in now:
                now[j] = carried[ip]
        for i in range(nl):           # published: a left keypoint with a stereo partner that exists
            j = int(stereo_idx[f, i])
            if not 0 <= j < nr:
                continue
            if i not in now:
                now[i] = next_id
                next_id += 1
            ids[f, i] = now[i]
            feat[f, i, 0], feat[f, i, 1] = normalised(kp_keys[2 * f, i], H, W)
            feat[f, i, 2], feat[f, i, 3] = normalised(kp_keys[2 * f + 1, j], H, W)
        carried = now
        for i, v in now.items():
            carried_out[f, i] = v
    return ids, feat, next_id, carried_out


def get_landmarks(ft, cam, Rt):
    """batch.py:152-166 for one feature (u0, v0, u1, v1): (world point [3], uL, uR, v)."""
    ft = np.asarray(ft, np.float64)
    cam = np.asarray(cam, np.float64)
    Rt = np.asarray(Rt, np.float64)
    fx, fy, cx, cy, baseline, res_x, res_y = cam[:7]
    with np.errstate(all="ignore"):
        f = (fx + fy) / 2.0
        uL = (ft[0] + 1) * 0.5 * res_x
        uR = (ft[2] + 1) * 0.5 * res_x
        v = ((ft[1] + ft[3]) / 2.0 + 1) * 0.5 * res_y
        d = uR - uL
        Wd = d / baseline
        xc, yc, zc = (uL - cx) / Wd, (v - cy) / Wd, f / Wd
        world = np.array([((Rt[3 * r] * xc + Rt[3 * r + 1] * yc) + Rt[3 * r + 2] * zc) + Rt[9 + r] for r in range(3)])
    return world, uL, uR, v


def emit_stereo_factors(ids, feat, Rt, cam, n_ids, first_frame):
    """batch_update's get_landmarks per keyframe and batch_create's landmark loop.  Returns a dict: obs_frame, obs_id,
    obs_meas (the factors in the order they are pushed), lm_first / lm_point per id below n_ids (-1 / zeros: never
    seen), frame_base [F+1] (factors pushed before each keyframe)."""
    ids = np.asarray(ids)
    F, K = ids.shape
    first, point = {}, {}
    obs_frame, obs_id, obs_meas = [], [], []
    frame_base = np.zeros(F + 1, np.int32)
    for f in range(F):
        frame_base[f] = len(obs_frame)
        if f < first_frame:
            continue
        for i in range(K):
            lid = int(ids[f, i])
            if not 0 <= lid < n_ids:
                continue
            world, uL, uR, v = get_landmarks(feat[f, i], cam, Rt[f])
            if lid not in first:              # `not initial_estimate.exists(L(id))`
                first[lid] = f * K + i
                point[lid] = world
            obs_frame.append(f)
            obs_id.append(lid)
            obs_meas.append((uL, uR, v))
    frame_base[F] = len(obs_frame)
    lm_first = np.full(n_ids, -1, np.int64)
    lm_point = np.zeros((n_ids, 3), np.float64)
    for lid, s in first.items():
        lm_first[lid] = s
        lm_point[lid] = point[lid]
    return dict(obs_frame=np.array(obs_frame, np.int32), obs_id=np.array(obs_id, np.int64),
                obs_meas=np.array(obs_meas, np.float64).reshape(-1, 3), lm_first=lm_first, lm_point=lm_point,
                frame_base=frame_base)


def stereo_initial_residuals(Rt, K6, lm_point, obs_frame, obs_id, obs_meas):
    """h(X(f), L(id)) - z of GenericStereoFactor3D, unwhitened: q = R^T (p - t), (cx + fx x / z, cx + fx (x - b) / z,
    cy + fy y / z) - (uL, uR, v); +inf in all three unless z > 0 (gtsam's cheirality case)."""
    Rt = np.asarray(Rt, np.float64).reshape(-1, 12)
    fx, fy, _, cx, cy, b = np.asarray(K6, np.float64)
    n = len(obs_frame)
    out = np.empty((n, 3), np.float64)
    with np.errstate(all="ignore"):
        for a in range(n):
            T, p, z_ = Rt[obs_frame[a]], lm_point[obs_id[a]], obs_meas[a]
            d0, d1, d2 = p[0] - T[9], p[1] - T[10], p[2] - T[11]
            x = (T[0] * d0 + T[3] * d1) + T[6] * d2
            y = (T[1] * d0 + T[4] * d1) + T[7] * d2
            z = (T[2] * d0 + T[5] * d1) + T[8] * d2
            if not z > 0.0:
                out[a] = np.inf
                continue
            out[a] = ((cx + fx * x / z) - z_[0], (cx + fx * (x - b) / z) - z_[1], (cy + fy * y / z) - z_[2])
    return out


def cross_check(idx_fwd, idx_bwd):
    """Keep the forward match i -> j only if the backward pairing matches j -> i."""
    idx_fwd, idx_bwd = np.asarray(idx_fwd), np.asarray(idx_bwd)
    P, K = idx_fwd.shape
    out = np.full((P, K), -1, np.int32)
    for p in range(P):
        for i in range(K):
            j = int(idx_fwd[p, i])
            if 0 <= j < K and int(idx_bwd[p, j]) == i:
                out[p, i] = j
    return out


def new_merged(n_img, max_kp, fill=0):
    """Merged per-image lists before the first level (kp_count zero, keys invalid); `fill` marks the untouched slots."""
    return dict(kp_keys=np.full((n_img, max_kp), 0xFFFFFFFF, np.uint32), kp_count=np.zeros(n_img, np.int32),
                desc=np.full((n_img, max_kp, 4), fill, np.uint64), angle=np.full((n_img, max_kp), fill, np.uint8),
                kp_level=np.full((n_img, max_kp), fill, np.uint8), kp_xy_q4=np.full((n_img, max_kp, 2), fill, np.int32))


def pyramid_append(lvl_keys, lvl_count, lvl_desc, lvl_angle, Hl, Wl, level, H0, W0, merged):
    """Append one level's keypoints to the merged lists (in place): the first min(count, capacity) of the level, as
    many as the merged list still has room for, positions mapped to level 0 in 1/16 pixel with pixel-centre alignment."""
    n_img, lvl_max_kp = lvl_keys.shape
    max_kp = merged["kp_keys"].shape[1]
    for n in range(n_img):
        base = int(merged["kp_count"][n])
        cnt = max(0, min(int(lvl_count[n]), lvl_max_kp, max_kp - base))
        for t in range(cnt):
            key = int(lvl_keys[n, t])
            pos = key & POS_MASK
            y, x = pos // Wl, pos % Wl
            xq = ((2 * x + 1) * 8 * W0 + Wl // 2) // Wl - 8
            yq = ((2 * y + 1) * 8 * H0 + Hl // 2) // Hl - 8
            x0 = min(max((xq + 8) >> 4, 0), W0 - 1)
            y0 = min(max((yq + 8) >> 4, 0), H0 - 1)
            o = base + t
            merged["kp_keys"][n, o] = (key & ~POS_MASK & 0xFFFFFFFF) | (y0 * W0 + x0)
            merged["desc"][n, o] = lvl_desc[n, t]
            merged["angle"][n, o] = lvl_angle[n, t]
            merged["kp_level"][n, o] = level
            merged["kp_xy_q4"][n, o] = (xq, yq)
        merged["kp_count"][n] = base + cnt
    return merged


def gate(resid, gate_px, obs_frame, obs_id, obs_meas, lm_first):
    """Keep a factor iff max |r| <= gate_px; a landmark survives iff a kept factor names it.  Returns (keep [n] bool,
    obs_frame, obs_id, obs_meas of the kept factors, lm_first with -1 for the landmarks that lost every factor)."""
    keep = np.array([bool(all(abs(v) <= gate_px for v in r)) for r in resid], bool).reshape(-1)
    named = {int(i) for i, k in zip(obs_id, keep) if k}
    first = np.array([s if lid in named else -1 for lid, s in enumerate(lm_first)], np.int64).reshape(-1)
    return keep, obs_frame[keep], obs_id[keep], obs_meas[keep], first


def same_bits(a, b):
    """Floats equal bit for bit, except that any NaN equals any NaN (infinities by sign, zeros by sign)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]))


# ======================================================================================================================
# generator

def make_tables(seed, F, K, H=480, W=640, p_stereo=0.6, p_track=0.7, p_collide=0.15, p_stale=0.08, p_oob=0.05,
                over=(), negative=(), no_left=(), no_right=(), full=False, chain=False):
    """Match tables of F stereo frames with K slots: dict(stereo_idx [F,K], track_idx [max(F-1,0),K], kp_keys [2F,K],
    kp_count [2F], H, W).  Every slot of every table is filled, beyond the counts too (a stale tail is what a
    reused buffer holds).
      p_stereo / p_track  share of entries that name an existing partner (the rest: -1, or the kinds below)
      p_collide           share of temporal entries that repeat the target of a lower-index keypoint
      p_stale             share of entries in [count, K): a partner slot that exists but holds no keypoint
      p_oob               share of temporal entries at or above K, or negative other than -1
      over / negative     image indices whose kp_count is above K / below zero
      no_left / no_right  frames whose left / right list is empty
      full                every list holds K keypoints;  chain: keypoint 0 -> 0 through every frame, always published."""
    rng = np.random.default_rng(seed)
    cnt = np.full(2 * F, K, np.int64) if full else rng.integers(K - K // 3, K + 1, 2 * F)
    for n in over:
        cnt[n] = K + 1 + 7 * (n % 3)
    for n in negative:
        cnt[n] = -3
    for f in no_left:
        cnt[2 * f] = 0
    for f in no_right:
        cnt[2 * f + 1] = 0
    eff = np.clip(cnt, 0, K)
    keys = ((rng.integers(0, 256, (2 * F, K)).astype(np.uint32) << 24) | rng.integers(0, H * W, (2 * F, K)).astype(np.uint32))

    def table(n_rows, n_target, p_match, collide, oob):
        """n_target[r]: existing partners of row r."""
        out = np.full((n_rows, K), -1, np.int64)
        for r in range(n_rows):
            u = rng.random(K)
            nt = int(n_target[r])
            if nt > 0:
                m = u < p_match
                out[r, m] = rng.integers(0, nt, int(m.sum()))
            if nt < K:
                m = (u >= p_match) & (u < p_match + p_stale)
                out[r, m] = rng.integers(nt, K, int(m.sum()))
            if oob:
                m = (u >= p_match + p_stale) & (u < p_match + p_stale + p_oob)
                out[r, m] = rng.choice([K, K + 3, 2 * K + 1, I32_MAX, -2, -K - 1, I32_MIN], int(m.sum()))
            if collide and K > 1:
                for i in np.nonzero(rng.random(K) < p_collide)[0]:
                    if i > 0:
                        out[r, i] = out[r, rng.integers(max(0, i - 4), i)]
        return out.astype(np.int32)

    stereo = table(F, eff[1::2], p_stereo, False, False)
    track = table(max(F - 1, 0), eff[2::2], p_track, True, True)
    if chain:
        stereo[:, 0] = 0
        if F > 1:
            track[:, 0] = 0
            track[:, 1:][track[:, 1:] == 0] = -1       # nobody else claims keypoint 0
    return dict(stereo_idx=stereo, track_idx=track, kp_keys=keys, kp_count=cnt.astype(np.int32), H=H, W=W)


def track_properties(t, ids, carried):
    """What a case of make_tables contains, counted from the tables and the reference's (ids, carried)."""
    stereo, track, cnt = t["stereo_idx"], t["track_idx"], t["kp_count"]
    F, K = stereo.shape
    eff = np.clip(cnt, 0, K)
    p = dict(collisions=0, collisions_idless_lowest=0, track_stale=0, track_oob=0, track_negative=0, stereo_stale=0,
             over_left=int((cnt[0::2] > K).sum()), over_right=int((cnt[1::2] > K).sum()), negative=int((cnt < 0).sum()),
             long_tracks=0, lost_tracks=0)
    for f in range(1, F):
        n_prev, nl = int(eff[2 * (f - 1)]), int(eff[2 * f])
        pred = {}
        for ip in range(n_prev):
            j = int(track[f - 1, ip])
            has_id = carried[f - 1, ip] >= 0
            if 0 <= j < nl:
                pred.setdefault(j, []).append(ip)
            elif has_id and nl <= j < K:
                p["track_stale"] += 1
            elif has_id and j >= K:
                p["track_oob"] += 1
            elif has_id and j < -1:
                p["track_negative"] += 1
        for j, ips in pred.items():
            if len(ips) >= 2:
                p["collisions"] += 1
                with_id = [ip for ip in ips if carried[f - 1, ip] >= 0]
                if with_id and with_id[0] != ips[0]:
                    p["collisions_idless_lowest"] += 1
    for f in range(F):
        nl, nr = int(eff[2 * f]), int(eff[2 * f + 1])
        p["stereo_stale"] += int(((stereo[f, :nl] >= nr) & (stereo[f, :nl] < K)).sum())
    seen = [set(ids[f][ids[f] >= 0].tolist()) for f in range(F)]
    if F:
        p["long_tracks"] = len(set.intersection(*seen))
        for f in range(F - 1):
            later = set().union(*seen[f + 1:])
            p["lost_tracks"] += len(seen[f] - later)
    return p


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_poses(rng, F, axis_aligned=()):
    """[F,12] row-major rotation then translation; the frames listed get the identity rotation (exact zeros)."""
    Rt = np.empty((F, 12))
    for f in range(F):
        Rt[f, :9] = (np.eye(3) if f in axis_aligned else random_rotation(rng)).reshape(-1)
        Rt[f, 9:] = rng.normal(size=3) * 2.0
    return Rt


CAM = np.array([1827.0, 1827.5999755859375, 968.9000244140625, 561.4000244140625, -0.063, 1920.0, 1080.0, 0.0])
K6 = np.array([1827.0, 1827.5999755859375, 0.0, 968.9000244140625, 561.4000244140625, 0.063])


def make_emission(seed, F, K, n_ids, density=0.6, empty=(), H=480, W=640, p_zero_disp=0.08, p_neg_disp=0.15):
    """A published-feature table as vus_track_ids would emit it, made adversarial: dict(ids [F,K] int64, feat [F,K,4],
    Rt [F,12], cam [8]).  Besides ids in [0, n_ids): -1, ids equal to n_ids and n_ids + 5, negative ids other than
    -1, the same id twice in a keyframe; keyframes in `empty` publish nothing.  Features sit on the pixel grid, so
    equal columns in both cameras (zero disparity) and a right column beyond the left one (the landmark behind the
    camera for this `cam`) occur exactly."""
    rng = np.random.default_rng(seed)
    ids = np.full((F, K), -1, np.int64)
    u = rng.random((F, K))
    if n_ids > 0:
        m = u < density
        ids[m] = rng.integers(0, n_ids, int(m.sum()))
    lo = density
    for val, share in ((n_ids, 0.04), (n_ids + 5, 0.04), (-2, 0.02), (-7, 0.02), (-2 ** 63, 0.02)):
        ids[(u >= lo) & (u < lo + share)] = val
        lo += share
    if K >= 8:                                # every kind in every keyframe, whatever the draw
        ids[:, 1], ids[:, 2], ids[:, 3], ids[:, 4] = n_ids, n_ids + 5, -2, -7
    if K >= 2 and n_ids > 0:
        for f in range(F):                    # the same id twice in one keyframe
            ids[f, K - 1] = ids[f, 0] = f % n_ids
    for f in empty:
        if 0 <= f < F:
            ids[f] = -1
    xl = rng.integers(40, W, (F, K))
    disp = rng.integers(1, 40, (F, K))
    kind = rng.random((F, K))
    disp[kind < p_zero_disp] = 0
    neg = (kind >= p_zero_disp) & (kind < p_zero_disp + p_neg_disp)
    disp[neg] = -np.minimum(disp[neg], W - 1 - xl[neg])
    xr = xl - disp
    yl = rng.integers(0, H, (F, K))
    yr = np.clip(yl + rng.integers(-2, 3, (F, K)), 0, H - 1)
    feat = np.stack([2.0 * xl / W - 1.0, 2.0 * yl / H - 1.0, 2.0 * xr / W - 1.0, 2.0 * yr / H - 1.0], axis=-1)
    return dict(ids=ids, feat=np.ascontiguousarray(feat), Rt=random_poses(rng, F), cam=CAM.copy())


def emission_properties(e, n_ids, first_frame, ref):
    ids, feat = e["ids"], e["feat"]
    F, K = ids.shape
    live = np.zeros((F, K), bool)
    live[first_frame:] = (ids[first_frame:] >= 0) & (ids[first_frame:] < n_ids)
    per_frame = live.sum(1)
    before = set(ids[:first_frame][(ids[:first_frame] >= 0) & (ids[:first_frame] < n_ids)].tolist())
    after = set(ids[live].tolist())
    dup = 0
    for f in range(F):
        v = ids[f][live[f]]
        dup += len(v) - len(set(v.tolist()))
    return dict(count=int(live.sum()), id_eq_n_ids=int((ids == n_ids).sum()), id_above=int((ids == n_ids + 5).sum()),
                id_negative=int((ids < -1).sum()), only_before_first=len(before - after), duplicates=dup,
                empty_start=bool(F and per_frame[0] == 0), empty_end=bool(F and per_frame[-1] == 0),
                empty_middle=bool((per_frame[1:-1] == 0).any()), never_seen=int((ref["lm_first"] < 0).sum()),
                zero_disparity=int((feat[..., 0] == feat[..., 2])[live].sum()),
                negative_disparity=int((feat[..., 2] > feat[..., 0])[live].sum()))


def make_residual_case(seed, n, n_frames=9, n_lm=50):
    """Factors for vus_stereo_initial_residuals with every cheirality case: dict(Rt, K6, lm_point, obs_frame, obs_id,
    obs_meas).  Frames 0 and 1 have the identity rotation, so that a landmark whose z equals the camera's lies on the
    camera plane EXACTLY (depth 0.0), and one with a smaller z behind it; some landmarks are non-finite, as the
    triangulation of a zero-disparity feature leaves them."""
    rng = np.random.default_rng(seed)
    Rt = random_poses(rng, n_frames, axis_aligned=(0, 1))
    pts = rng.normal(size=(n_lm, 3)) * 4.0
    pts[0, 2], pts[1, 2], pts[2, 2] = Rt[0, 11], Rt[1, 11], Rt[0, 11] - 1.5        # on the plane of frame 0 / 1, behind 0
    pts[3] = (np.inf, -np.inf, np.inf)
    pts[4] = (np.nan, 1.0, 2.0)
    pts[5] = (1.0, np.nan, np.inf)
    obs_frame = rng.integers(0, n_frames, n).astype(np.int32)
    obs_id = rng.integers(0, n_lm, n).astype(np.int64)
    k = min(n, 30)                      # the designed rows first: plane of frame 0, plane of frame 1, behind, non-finite
    obs_frame[:k] = np.array([0, 1, 0, 2, 3, 4] * 5, np.int32)[:k]
    obs_id[:k] = np.array([0, 1, 2, 3, 4, 5] * 5, np.int64)[:k]
    obs_meas = np.ascontiguousarray(rng.uniform(0, 1900, (n, 3)))
    return dict(Rt=Rt, K6=K6.copy(), lm_point=pts, obs_frame=obs_frame, obs_id=obs_id, obs_meas=obs_meas)


def residual_properties(c, resid):
    """Depth classes of the factors, with the depth recomputed here in exact identity-frame arithmetic."""
    inf_rows = np.isposinf(resid).all(1)
    on_plane = 0
    for a in range(len(c["obs_frame"])):
        f, lid = int(c["obs_frame"][a]), int(c["obs_id"][a])
        if f in (0, 1) and c["lm_point"][lid, 2] == c["Rt"][f, 11] and np.isfinite(c["lm_point"][lid]).all():
            on_plane += 1
    return dict(inf_rows=int(inf_rows.sum()), on_plane=on_plane,
                nonfinite_points=int((~np.isfinite(c["lm_point"][c["obs_id"]]).all(1)).sum()),
                finite_rows=int(np.isfinite(resid).all(1).sum()), mixed_rows=int((np.isinf(resid).any(1) & ~inf_rows).sum()))


def make_cross_check(seed, P, K):
    """Forward / backward pairings [P,K]: about half the forward matches mutual, the rest one-sided, -1, or out of
    range on either side of K."""
    rng = np.random.default_rng(seed)
    fwd = rng.integers(-1, K + 3, (P, K)).astype(np.int32)
    bwd = rng.integers(-1, K + 3, (P, K)).astype(np.int32)
    for p in range(P):
        for i in range(K):
            j = int(fwd[p, i])
            if 0 <= j < K and rng.random() < 0.5:
                bwd[p, j] = i
    return fwd, bwd


# level sizes that are no integer ratio of level 0 (a x1.2 pyramid of 120 x 160)
PYR_SIZES = [(120, 160), (100, 133), (83, 111), (69, 92)]
PYR_MAX_KP, PYR_LVL_MAX_KP = 45, 48
# per image, the count each level reports: normal; a zero level and one equal to what is left (35 after 10);
# the whole quota from level 0 (45 == max_kp, so later levels meet a full list); above the level's capacity (60 > 48);
# above what is left (30 > 25)
PYR_COUNTS = np.array([[7, 5, 3, 2], [10, 0, 35, 4], [45, 9, 9, 9], [60, 3, 3, 3], [20, 30, 5, 1]], np.int32)


def make_pyramid_levels(seed, n_levels):
    """Per level: (keys [n_img, lvl_max_kp], count [n_img], desc, angle, Hl, Wl); every slot filled, beyond the count too."""
    rng = np.random.default_rng(seed)
    n_img = len(PYR_COUNTS)
    out = []
    for lv in range(n_levels):
        Hl, Wl = PYR_SIZES[lv]
        keys = ((rng.integers(0, 256, (n_img, PYR_LVL_MAX_KP)).astype(np.uint32) << 24) |
                rng.integers(0, Hl * Wl, (n_img, PYR_LVL_MAX_KP)).astype(np.uint32))
        keys[:, 0] = (np.uint32(200) << 24) | np.uint32(Hl * Wl - 1)          # the last pixel: the clamp to W0-1, H0-1
        keys[:, 1] = np.uint32(201) << 24                                     # the first pixel
        desc = rng.integers(0, 2 ** 63, (n_img, PYR_LVL_MAX_KP, 4)).astype(np.uint64)
        ang = rng.integers(0, 30, (n_img, PYR_LVL_MAX_KP)).astype(np.uint8)
        out.append((keys, PYR_COUNTS[:, lv].copy(), desc, ang, Hl, Wl))
    return out


# ======================================================================================================================
# the cases both test files run, each built (and its reference computed) once per session

TRACK_MAX_KP = [1, 63, 1023, 1024, 1025, 2047, 2049, 4097, 7986, 7987, 8192]
TRACK_CASES = {f"max_kp{K}": dict(seed=K, F=5, K=K, over=(2, 5)) for K in TRACK_MAX_KP}
TRACK_CASES.update({f"frames{F}": dict(seed=50 + F, F=F, K=300, chain=F == 40) for F in (0, 1, 2, 40)})
TRACK_CASES["odd_image"] = dict(seed=7, F=5, K=300, H=203, W=97)
TRACK_CASES["full_lists"] = dict(seed=8, F=4, K=1025, full=True, p_stale=0.0)
# counts above K on both sides, a negative count (frame 7's left list), an empty left list (frame 3) and an empty
# right list (frame 5) in mid-sequence
TRACK_CASES["adversarial"] = dict(seed=9, F=9, K=400, over=(0, 3), negative=(14,), no_left=(3,), no_right=(5,))

EMIT_CASES = {f"max_kp{K}": dict(seed=K, F=6, K=K, n_ids=2 * K + 3, first_frame=1) for K in (1, 255, 256, 257, 2049)}
EMIT_CASES.update({f"frames{F}": dict(seed=F, F=F, K=5, n_ids=200, first_frame=1, empty=(0, F // 2, F - 1))
                   for F in (1, 1023, 1024, 1025, 2049, 5000)})
EMIT_CASES.update({f"first{ff}": dict(seed=60 + ff, F=6, K=40, n_ids=90, first_frame=ff, empty=(0, 3, 5))
                   for ff in (0, 1, 3, 6, 8)})
EMIT_CASES.update({f"n_ids{n}": dict(seed=70 + n, F=6, K=40, n_ids=n, first_frame=1) for n in (0, 1, 90)})
# few landmarks seen many times, a third of the sightings behind the camera: what the gate tests filter
EMIT_CASES["dense"] = dict(seed=90, F=8, K=60, n_ids=40, first_frame=1, p_neg_disp=0.3)
EMIT_CASES["all_empty"] = dict(seed=80, F=6, K=40, n_ids=90, first_frame=1, empty=tuple(range(6)))

RESIDUAL_N = [0, 1, 255, 256, 257, 10000]
CROSS_CHECK_CASES = [(P, K) for K in (1, 257) for P in (0, 1, 7)]

_cache = {}


def track_case(name):
    """(tables, (ids, feat, n_ids, carried) of the reference)."""
    if ("track", name) not in _cache:
        t = make_tables(**TRACK_CASES[name])
        _cache["track", name] = (t, track_ids(t["stereo_idx"], t["track_idx"], t["kp_keys"], t["kp_count"], t["H"], t["W"]))
    return _cache["track", name]


def emit_case(name):
    """(emission tables, n_ids, first_frame, the reference's factors)."""
    if ("emit", name) not in _cache:
        c = dict(EMIT_CASES[name])
        n_ids, ff = c.pop("n_ids"), c.pop("first_frame")
        e = make_emission(**c, n_ids=n_ids)
        _cache["emit", name] = (e, n_ids, ff, emit_stereo_factors(e["ids"], e["feat"], e["Rt"], e["cam"], n_ids, ff))
    return _cache["emit", name]


def residual_case(n):
    """(factors, the reference's residuals)."""
    if ("resid", n) not in _cache:
        c = make_residual_case(1000 + n, n)
        _cache["resid", n] = (c, stereo_initial_residuals(c["Rt"], c["K6"], c["lm_point"], c["obs_frame"], c["obs_id"],
                                                          c["obs_meas"]))
    return _cache["resid", n]


def gate_thresholds(resid, obs_id):
    """The gates a case is filtered with, chosen from the reference's residuals alone: dict(name -> gate_px).
    `all` keeps every factor whose residual is a number, `none` keeps nothing, and `first_dropped` is the largest
    residual of some factor -- so that factor sits exactly ON the gate and must be kept -- picked such that some
    landmark loses its first sighting and keeps a later one (absent if the case has no such landmark)."""
    m = np.array([max(abs(v) for v in r) if not np.isnan(r).any() else np.nan for r in resid], np.float64).reshape(-1)
    out = {"all": float("inf"), "finite": 1e308, "none": -1.0}
    first = {}
    for a, lid in enumerate(obs_id):
        first.setdefault(int(lid), a)
    for g in np.unique(m[np.isfinite(m)]):
        keep = m <= g
        if any(keep[a] and not keep[first[int(lid)]] for a, lid in enumerate(obs_id)):
            out["first_dropped"] = float(g)
            break
    return out
