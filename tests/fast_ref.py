"""Plain numpy reference of the FAST detector (include/vus.h), written from the header's definitions and not from the
oracle's loops, plus a deterministic set of adversarial images for it.  Test infrastructure only (a plain module, not
a conftest).

Every function takes images as [n, H, W] uint8 (any strides: a padded buffer's [:, :, :W] view is fine) and works in
exact integer arithmetic, vectorised over the 16 circle offsets."""
import numpy as np

# FAST circle, clockwise from 12 o'clock (include/vus_orb_tables.h), and the 7-tap smoothing weights (sum 256)
CIRCLE_DX = np.array([0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1])
CIRCLE_DY = np.array([-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3])
ARC = 9
BLUR_W = np.array([18, 33, 49, 56, 49, 33, 18], np.int64)
KEY_INVALID = 0xFFFFFFFF
TILE_W, TILE_H = 128, 24          # VUS_FAST_TILE_W / _H
SAMPLE_FLOOR = 40                 # VUS_FAST_SAMPLE_FLOOR
MARGIN_NUM, MARGIN_DEN = 7, 4     # VUS_FAST_MARGIN_NUM / _DEN


def _as3(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8
    return img[None] if img.ndim == 2 else img


def fast_score(img, thr):
    """score(y, x) = max(best bright arc, -best dark arc) - 1 over the 16 arcs of 9, where an arc's bright side is the
    min of d and its dark side the max of d (d = circle pixel - centre); written where score >= thr, else 0; the
    3-pixel frame is 0.  uint8 [n, H, W]."""
    img = _as3(img)
    n, H, W = img.shape
    out = np.zeros((n, H, W), np.uint8)
    if H < 7 or W < 7:
        return out
    im = img.astype(np.int16)
    c = im[:, 3:H - 3, 3:W - 3]
    d = np.stack([im[:, 3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in zip(CIRCLE_DX, CIRCLE_DY)])
    bright = np.full(c.shape, -256, np.int16)           # max over the arcs of the arc's min d
    dark = np.full(c.shape, 256, np.int16)              # min over the arcs of the arc's max d
    for start in range(16):
        arc = d[(start + np.arange(ARC)) & 15]
        bright = np.maximum(bright, arc.min(axis=0))
        dark = np.minimum(dark, arc.max(axis=0))
    s = np.maximum(bright, -dark).astype(np.int32) - 1
    out[:, 3:H - 3, 3:W - 3] = np.where(s >= thr, s, 0).astype(np.uint8)
    return out


def nms_survivors(score, border):
    """Strict 3x3 maximum over a thresholded score map (outside the image counts as 0), then the border filter:
    bool [n, H, W]."""
    n, H, W = score.shape
    s = score.astype(np.int16)
    p = np.zeros((n, H + 2, W + 2), np.int16)
    p[:, 1:-1, 1:-1] = s
    m = np.zeros_like(s)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m = np.maximum(m, p[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx])
    keep = (s > 0) & (s > m)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    inside = (ys >= border) & (ys < H - border) & (xs >= border) & (xs < W - border)
    return keep & inside[None]


def keys_of(score, keep):
    """Per image: the sorted keys (255 - s) << 24 | (y W + x) of the kept pixels (uint32)."""
    n, H, W = score.shape
    out = []
    for i in range(n):
        pos = np.flatnonzero(keep[i])
        k = ((255 - score[i].reshape(-1)[pos].astype(np.uint32)) << np.uint32(24)) | pos.astype(np.uint32)
        out.append(np.sort(k))
    return out


def fast_detect(img, thr, border):
    """(list of per-image sorted candidate keys, true counts [n] int32) of FAST + strict 3x3 NMS + border filter."""
    img = _as3(img)
    sc = fast_score(img, thr)
    keys = keys_of(sc, nms_survivors(sc, border))
    return keys, np.array([len(k) for k in keys], np.int32)


def blur7(img):
    """7x7 separable smoothing, replicate borders: exact row sums H = sum w img, then (sum w H + 32768) >> 16."""
    img = _as3(img)
    n, H, W = img.shape
    x = np.clip(np.arange(W)[:, None] + np.arange(-3, 4)[None, :], 0, W - 1)      # [W, 7]
    y = np.clip(np.arange(H)[:, None] + np.arange(-3, 4)[None, :], 0, H - 1)      # [H, 7]
    hs = (img.astype(np.int64)[:, :, x] * BLUR_W).sum(axis=-1)                      # [n, H, W]
    vs = (hs[:, y, :] * BLUR_W[None, None, :, None]).sum(axis=2)                    # [n, H, W]
    return ((vs + 32768) >> 16).astype(np.uint8)


def select_topk(keys, max_kp):
    """keys: per-image candidate key arrays (the first min(count, cap) of a list, any order).  The max_kp smallest,
    ascending, tail VUS_KEY_INVALID: (kp [n, max_kp] uint32, kp_count [n] int32)."""
    kp = np.full((len(keys), max_kp), KEY_INVALID, np.uint32)
    cnt = np.zeros(len(keys), np.int32)
    for i, k in enumerate(keys):
        k = np.sort(np.asarray(k, np.uint32))[:max_kp]
        kp[i, :len(k)] = k
        cnt[i] = len(k)
    return kp, cnt


def tile_counts(H, W, stride):
    """(tiles_x, n_tiles, n_sampled) of the estimate's 128 x 24 raster tiles."""
    tx, ty = -(-W // TILE_W), -(-H // TILE_H)
    n_tiles = tx * ty
    n_sampled = max(1, -(-(n_tiles - stride // 2) // stride))
    return tx, n_tiles, n_sampled


def threshold_estimate(img, thr, border, max_kp, stride):
    """(hist [n, 256] int32, thr_img [n] int32) of vus_fast_threshold_estimate: the survivors with score >= f =
    max(thr, 40) in the sampled tiles (tile >= stride / 2, (tile - stride / 2) % stride == 0) binned by score;
    thr_img = the largest t in (f, 254] with count(score >= t) * n_tiles * 4 >= max_kp * n_sampled * 7, else thr."""
    img = _as3(img)
    n, H, W = img.shape
    tx, n_tiles, n_sampled = tile_counts(H, W, stride)
    f = max(thr, SAMPLE_FLOOR)
    sc = fast_score(img, thr)
    keep = nms_survivors(sc, border)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    tile = (ys // TILE_H) * tx + xs // TILE_W
    sampled = (tile >= stride // 2) & ((tile - stride // 2) % stride == 0)
    hist = np.zeros((n, 256), np.int32)
    thr_img = np.zeros(n, np.int32)
    for i in range(n):
        s = sc[i][keep[i] & sampled & (sc[i] >= f)]
        hist[i] = np.bincount(s, minlength=256)[:256]
        run = np.cumsum(hist[i][::-1].astype(np.int64))[::-1]       # run[t] = count(score >= t)
        ok = [t for t in range(f + 1, 255) if run[t] * n_tiles * MARGIN_DEN >= max_kp * n_sampled * MARGIN_NUM]
        thr_img[i] = max(ok) if ok else thr
    return hist, thr_img


# ---------------------------------------------------------------------------------------------------------------------
# Adversarial images.  Every generator is deterministic (fixed seeds) and returns uint8 [n, H, W].

ARC_LENGTHS = (7, 8, 9, 10, 12, 16)


def stamp_list(thr):
    """(L, k, sign, delta) of every arc stamp: arcs of length L from every start k, both polarities, contrasts
    thr - 1 .. thr + 2."""
    return [(L, k, sgn, dl) for L in ARC_LENGTHS for k in range(16) for sgn in (1, -1)
            for dl in (thr - 1, thr, thr + 1, thr + 2)]


def stamp_centres(H, W, count):
    """Up to `count` stamp centres on an 8-pixel grid whose x phase sweeps x mod 4 row by row, starting at the first
    interior pixel (3 from the top / left edge); at H = 192, W = 259 the last row and column lie 4 and 3 pixels from
    the bottom / right edge."""
    out = []
    for r, y in enumerate(range(3, H - 3, 8)):
        for x in range(3 + (r % 4), W - 3, 8):
            out.append((y, x))
    return out[:count]


def arc_stamp_image(H, W, c, stamps):
    """A flat image at c with the given arc stamps on the grid of stamp_centres: ring at c except the arc, which is
    at clamp(c + sign * delta).  Returns (image [H, W], [(y, x, L, k, sign, delta), ...]) for the stamps laid."""
    img = np.full((H, W), c, np.uint8)
    laid = []
    for (y, x), (L, k, sgn, dl) in zip(stamp_centres(H, W, len(stamps)), stamps):
        v = int(np.clip(c + sgn * dl, 0, 255))
        for j in range(L):
            q = (k + j) & 15
            img[y + CIRCLE_DY[q], x + CIRCLE_DX[q]] = v
        laid.append((y, x, L, k, sgn, dl))
    return img, laid


def stamp_centre_score(c, L, sgn, dl):
    """The definition's answer at a stamp centre: an arc of 9 exists only for L >= 9, and its contrast is the clamped one."""
    eff = abs(int(np.clip(c + sgn * dl, 0, 255)) - c)
    return eff - 1 if L >= ARC and eff > 0 else -1


def stamp_centre_values(thr):
    return (0, 1, thr, 127, 128, 255 - thr, 254, 255)


def arc_stamp_images(thr, H=192, W=259):
    """One image per centre value c in {0, 1, thr, 127, 128, 255 - thr, 254, 255}, all stamps of stamp_list(thr);
    192 x 259 holds exactly the 768 stamps, crosses the x = 128 k / y = 24 k tile edges and has W % 4 = 3."""
    imgs, lays = [], []
    for c in stamp_centre_values(thr):
        im, laid = arc_stamp_image(H, W, c, stamp_list(thr))
        imgs.append(im); lays.append(laid)
    return np.stack(imgs), lays


def saturated_images(H, W, thr, seed=0):
    """Binary 0/255 at densities 0.5, 0.1, 0.02; salt-and-pepper on grounds 0, 128, 255; uniform noise; +-(thr + 1)
    noise around 128."""
    rng = np.random.default_rng(seed)
    out = [np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8) for p in (0.5, 0.1, 0.02)]
    for g in (0, 128, 255):
        u = rng.random((H, W))
        im = np.full((H, W), g, np.uint8)
        im[u < 0.05] = 0
        im[u > 0.95] = 255
        out.append(im)
    out.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
    out.append(np.clip(128 + (thr + 1) * rng.integers(-1, 2, (H, W)), 0, 255).astype(np.uint8))
    return np.stack(out)


def plateau_images(H, W, lo=0, hi=255):
    """Checkerboards and stripes of period 1..5 in x, y and along the diagonal (two levels lo / hi)."""
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    out = []
    for p in range(1, 6):
        for f in ((xs // p + ys // p) % 2, (xs // p) % 2 + 0 * ys, (ys // p) % 2 + 0 * xs, ((xs + ys) // p) % 2):
            out.append(np.where(f == 1, hi, lo).astype(np.uint8))
    return np.stack(out)


def tie_image(H, W, thr, c=100, step=8):
    """One bright corner (arc of 9 from k = 0, contrast thr + 5) repeated on a grid of `step` pixels: hundreds of
    equal scores, every stamp centre a survivor."""
    im = np.full((H, W), c, np.uint8)
    v = min(255, c + thr + 5)
    for y in range(4, H - 4, step):
        for x in range(4, W - 4, step):
            for j in range(ARC):
                im[y + CIRCLE_DY[j], x + CIRCLE_DX[j]] = v
    return im


def corner_free_images(H, W, thr):
    """Constant 0 and 255, and x / y ramps of step 1 and step thr (clamped at 255): every arc of 9 holds a pixel of
    the ramp's own row or column (d = 0), so nothing is a corner although near-threshold differences are everywhere."""
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    out = [np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]
    for step in (1, thr):
        out.append(np.minimum(xs * step + 0 * ys, 255).astype(np.uint8))
        out.append(np.minimum(ys * step + 0 * xs, 255).astype(np.uint8))
    return np.stack(out)


def concentrated_image(H, W, col=3, seed=0, flat=80):
    """A flat image with uniform noise in one 128-pixel tile column: every candidate lands in the tiles of one
    candidate sub-list when tiles_x is a multiple of 8 (widths 897 .. 1024)."""
    im = np.full((H, W), flat, np.uint8)
    col = min(col, (W - 1) // TILE_W)
    x0, x1 = TILE_W * col, min(W, TILE_W * (col + 1))
    im[:, x0:x1] = np.random.default_rng(seed).integers(0, 256, (H, x1 - x0), dtype=np.uint8)
    return im


def pitches(W):
    """The row pitches every entry point is checked at: W, W + 1, W + 13 and the next multiple of 64 above W."""
    return sorted({W, W + 1, W + 13, (W // 64 + 1) * 64})


def pitch_at(W, k):
    """The k-th of pitches(W), cyclically (there are three when W + 1 or W + 13 is the multiple of 64)."""
    p = pitches(W)
    return p[k % len(p)]


def padded(img, pitch):
    """[n, H, pitch] buffer holding img in its first W columns and alternating 0 / 255 junk in the padding."""
    img = _as3(img)
    n, H, W = img.shape
    buf = np.empty((n, H, pitch), np.uint8)
    junk = np.where((np.arange(H)[:, None] + np.arange(pitch)[None, :]) % 2 == 0, 0, 255).astype(np.uint8)
    buf[:] = junk
    buf[:, :, :W] = img
    return buf
