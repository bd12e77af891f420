"""Plain numpy statement of vus_stereo_refine (include/vus_subpixel.h), of the Q8 candidate rule of
vus_stereo_pair_pose_q8 (include/vus_loop.h) and of the u1 formula of frontend.feature_tracks(disparity=...).  Test
infrastructure only (a plain module, not a conftest).

Everything in refine() is integer arithmetic in int64, stated operation by operation as the header states it, vectorised
over the matched slots of a frame; the outputs are cast to the ABI's int32 / uint8 at the end (an int32 wrap, as the
kernel's).  The kernel must EQUAL it word for word."""
import numpy as np

import loop_ref as L
import track_ref as T

OK, EDGE, NONE = 0, 1, 255
MAX_HALF_WIN, MAX_SEARCH = 7, 8


def floor_div(a, b):
    """Mathematical floor of a / b for b > 0 (numpy's // on integers is floor division; stated for the reader)."""
    return np.asarray(a, np.int64) // np.asarray(b, np.int64)


def fit_q(cm, c0, cp):
    """q of the header's REFINEMENT from the three costs around the minimum (arrays or scalars), int64."""
    cm, c0, cp = (np.asarray(v, np.int64) for v in (cm, c0, cp))
    m = np.maximum(cm, cp) - c0
    safe = np.where(m == 0, 1, m)
    return np.where(m == 0, 0, floor_div(256 * (cm - cp) + m, 2 * safe))


def costs(Limg, Rimg, xl, yl, xr, H, W, half_win, search):
    """cost(s) for s = -search .. search of n matches: int64 [n, 2 search + 1].  Limg, Rimg: [H, >= W] uint8; xl, yl, xr
    int64 [n].  Replicate border: every coordinate is clamped."""
    Li, Ri = Limg.astype(np.int64), Rimg.astype(np.int64)
    d = np.arange(-half_win, half_win + 1)
    ys = np.clip(yl[:, None] + d[None, :], 0, H - 1)                                   # [n, win]
    xls = np.clip(xl[:, None] + d[None, :], 0, W - 1)
    lw = Li[ys[:, :, None], xls[:, None, :]]                                           # [n, win(dy), win(dx)]
    out = np.zeros((len(xl), 2 * search + 1), np.int64)
    for k, s in enumerate(range(-search, search + 1)):
        xrs = np.clip(xr[:, None] + s + d[None, :], 0, W - 1)
        out[:, k] = np.abs(lw - Ri[ys[:, :, None], xrs[:, None, :]]).sum((1, 2))
    return out


def matched(stereo_idx, kp_count, f):
    """(i, j) int64 arrays of the matched slots of frame f, by the header's SLOT RULE."""
    K = stereo_idx.shape[1]
    nl, nr = T._clamp_count(kp_count[2 * f], K), T._clamp_count(kp_count[2 * f + 1], K)
    i = np.arange(nl)
    j = stereo_idx[f, :nl].astype(np.int64)
    ok = (j >= 0) & (j < nr)
    return i[ok], j[ok]


def positions(kp_keys, f, i, j, W):
    """(xl, yl, xr) int64 of the matched slots."""
    keys = np.asarray(kp_keys).view(np.uint32).astype(np.int64)
    p, q = keys[2 * f, i] & T.POS_MASK, keys[2 * f + 1, j] & T.POS_MASK
    yl = p // W
    return p - yl * W, yl, q - (q // W) * W


def refine(img, W, stereo_idx, kp_keys, kp_count, half_win, search, return_costs=False):
    """vus_stereo_refine: img uint8 [2F, H, pitch >= W]; returns (disp_q8 int32 [F,K], status uint8 [F,K])."""
    assert 1 <= half_win <= MAX_HALF_WIN and 1 <= search <= MAX_SEARCH
    stereo_idx = np.asarray(stereo_idx)
    F, K = stereo_idx.shape
    H = img.shape[1]
    disp = np.zeros((F, K), np.int64)
    status = np.full((F, K), NONE, np.uint8)
    all_costs = []
    for f in range(F):
        i, j = matched(stereo_idx, kp_count, f)
        if not len(i):
            all_costs.append(np.zeros((0, 2 * search + 1), np.int64))
            continue
        xl, yl, xr = positions(kp_keys, f, i, j, W)
        d0 = xl - xr
        c = costs(img[2 * f], img[2 * f + 1], xl, yl, xr, H, W, half_win, search)
        all_costs.append(c)
        k = np.argmin(c, axis=1)                                   # the first of equal minima: the lowest s
        edge = (k == 0) | (k == 2 * search)
        kk = np.clip(k, 1, 2 * search - 1)
        n = np.arange(len(i))
        q = fit_q(c[n, kk - 1], c[n, kk], c[n, kk + 1])
        disp[f, i] = np.where(edge, 256 * d0, 256 * (d0 - (k - search)) - q)
        status[f, i] = np.where(edge, EDGE, OK)
    out = (disp & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return (out, status, all_costs) if return_costs else (out, status)


def integer_disparity_q8(stereo_idx, kp_keys, kp_count, W):
    """256 d0 on the matched slots, 0 elsewhere: the Q8 form of today's integer disparities, int32 [F,K]."""
    stereo_idx = np.asarray(stereo_idx)
    F, K = stereo_idx.shape
    out = np.zeros((F, K), np.int32)
    for f in range(F):
        i, j = matched(stereo_idx, kp_count, f)
        xl, _, xr = positions(kp_keys, f, i, j, W)
        out[f, i] = 256 * (xl - xr)
    return out


def u1(xl, disp_q8, W):
    """The normalised right column of a feature from its left column and refined disparity: xr = (256 xl - disp_q8) / 256.0
    is exact in f64; then the statement of vus_track_ids, 2.0 * xr / W - 1.0."""
    xr = (256 * np.asarray(xl, np.int64) - np.asarray(disp_q8, np.int64)).astype(np.float64) / 256.0
    return 2.0 * xr / np.float64(W) - 1.0


def candidates_q8(t, c, disp_q8):
    """loop_ref.candidates with the Q8 rule of vus_stereo_pair_pose_q8: (src, dst, x1, y1, d1, x2, y2, d2), d1 and d2
    float64 = disp_q8 / 256.0."""
    K, W, Fn = t["match_idx"].shape[1], t["W"], len(t["stereo_idx"])
    a, b = int(t["pair_a"][c]), int(t["pair_b"][c])
    empty = (np.zeros(0, np.int64),) * 8
    if not (0 <= a < Fn and 0 <= b < Fn and a != b):
        return empty
    nla, nra, nlb, nrb = (T._clamp_count(t["kp_count"][q], K) for q in (2 * a, 2 * a + 1, 2 * b, 2 * b + 1))
    i = np.arange(nla)
    j = t["match_idx"][c, :nla].astype(np.int64)
    ok = (j >= 0) & (j < nlb)
    i, j = i[ok], j[ok]
    sa, sb = t["stereo_idx"][a, i].astype(np.int64), t["stereo_idx"][b, j].astype(np.int64)
    ok = (sa >= 0) & (sa < nra) & (sb >= 0) & (sb < nrb)
    i, j = i[ok], j[ok]
    x1, y1 = L.decode(t["kp_keys"][2 * a, i], W)
    x2, y2 = L.decode(t["kp_keys"][2 * b, j], W)
    q1, q2 = disp_q8[a, i].astype(np.int64), disp_q8[b, j].astype(np.int64)
    ok = (q1 >= 256) & (q2 >= 256)
    d1, d2 = q1.astype(np.float64) / 256.0, q2.astype(np.float64) / 256.0
    return i[ok], j[ok], x1[ok], y1[ok], d1[ok], x2[ok], y2[ok], d2[ok]


def stereo_pair_pose_q8(t, disp_q8, threshold_px, n_hyp, seed, refine_iters, mg=None):
    """vus_stereo_pair_pose_q8 on a table dict: loop_ref.stereo_pair_pose with candidates_q8; pair_pose is unchanged."""
    disp_q8 = np.asarray(disp_q8)
    Pn, K = t["match_idx"].shape
    res = dict(T_ab=np.zeros((Pn, 12)), JtJ=np.zeros((Pn, 36)), rss=np.zeros(Pn), match_idx_out=np.full((Pn, K), -1, np.int32),
               info=np.zeros((Pn, 6), np.int32))
    for c in range(Pn):
        src, dst, *cand = candidates_q8(t, c, disp_q8)
        o = L.pair_pose(*cand, t["cam"], threshold_px, n_hyp, seed, c, refine_iters, mg)
        res["T_ab"][c], res["JtJ"][c], res["rss"][c], res["info"][c] = o["T"], o["JtJ"].reshape(-1), o["rss"], o["info"]
        res["match_idx_out"][c, src[o["keep"]]] = dst[o["keep"]]
    return res
