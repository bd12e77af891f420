"""The numpy statement of contrast-limited adaptive histogram equalisation (include/vus_clahe.h), written
from the contract and independently of the kernels and of visual_underwater_slam_amd/clahe.py (which imports nothing from
here): the integer statement the GPU equals bit for bit, a float32 restatement of the textbook / OpenCV formula it is
compared with, and the "murk" image model of the tests.

Test infrastructure only."""
import numpy as np

MAX_TILES, MAX_TILE_PIXELS = 32, 1 << 22


def tile_size(H, W, tx, ty):
    """(tw, th) of the contract; ValueError where the contract refuses the call."""
    if not (1 <= H <= 32767 and 1 <= W <= 32767):
        raise ValueError(f"H={H} W={W} outside 1..32767")
    if not (1 <= tx <= MAX_TILES and 1 <= ty <= MAX_TILES):
        raise ValueError(f"tiles_x={tx} tiles_y={ty} outside 1..{MAX_TILES}")
    tw, th = -(-W // tx), -(-H // ty)
    if ty * th - H > H - 1 or tx * tw - W > W - 1:
        raise ValueError("the padding is larger than reflect-101 can fill")
    if tw * th > MAX_TILE_PIXELS:
        raise ValueError("T above 2^22")
    return tw, th


def clip_count(clip_limit, T):
    """OpenCV's rule, in double precision."""
    return max(1, int(float(clip_limit) * T / 256.0)) if clip_limit > 0 else 0


def _reflect(n, total):
    idx = np.arange(total)
    return np.where(idx < n, idx, 2 * (n - 1) - idx)


def tile_histograms(img, tx, ty):
    """int64 [n, ty, tx, 256]: the histograms of the padded tiles of img uint8 [n, H, W]."""
    img = np.asarray(img)
    n, H, W = img.shape
    tw, th = tile_size(H, W, tx, ty)
    pad = img[:, _reflect(H, ty * th)][:, :, _reflect(W, tx * tw)]
    tiles = pad.reshape(n, ty, th, tx, tw).transpose(0, 1, 3, 2, 4).reshape(n * ty * tx, th * tw).astype(np.int64)
    ids = tiles + 256 * np.arange(n * ty * tx, dtype=np.int64)[:, None]
    return np.bincount(ids.reshape(-1), minlength=n * ty * tx * 256).reshape(n, ty, tx, 256)


def clip_histograms(h, clip):
    """Step 2 of the contract on int64 [..., 256]."""
    h = np.asarray(h, np.int64)
    if clip <= 0:
        return h.copy()
    excess = np.maximum(h - clip, 0).sum(-1, keepdims=True)
    out = np.minimum(h, clip) + excess // 256
    r = excess % 256
    step = np.maximum(256 // np.maximum(r, 1), 1)
    b = np.arange(256, dtype=np.int64)
    return out + ((r > 0) & (b % step == 0) & (b // step < r))


def luts(img, tx, ty, clip):
    """uint8 [n, ty, tx, 256] of img uint8 [n, H, W] (or [H, W]: n = 1)."""
    img = np.asarray(img)
    img = img[None] if img.ndim == 2 else img
    tw, th = tile_size(img.shape[1], img.shape[2], tx, ty)
    T = tw * th
    c = np.cumsum(clip_histograms(tile_histograms(img, tx, ty), int(clip)), axis=-1)
    out = (c * 255 + T // 2) // T
    assert (out[..., 255] == 255).all()
    return out.astype(np.uint8)


def axis_weights(n, t, tiles):
    """(i1, i2, w) int64 [n] of the contract's interpolation along an axis of n pixels with tile size t."""
    p = 2 * np.arange(n, dtype=np.int64) - t
    t1 = p // (2 * t)                                     # floor
    a = p - t1 * 2 * t
    assert (a >= 0).all() and (a < 2 * t).all()
    return np.clip(t1, 0, tiles - 1), np.clip(t1 + 1, 0, tiles - 1), (a * 256 + t) // (2 * t)


def apply(img, lut, tx, ty):
    """uint8 [n, H, W]: img uint8 [n, H, W] through lut uint8 [n, ty, tx, 256] (any bytes, not only those of luts())."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    img = img[None] if squeeze else img
    n, H, W = img.shape
    tw, th = tile_size(H, W, tx, ty)
    lut = np.asarray(lut).reshape(n, ty, tx, 256).astype(np.int64)
    x1, x2, wx = (v[None, None, :] for v in axis_weights(W, tw, tx))
    y1, y2, wy = (v[None, :, None] for v in axis_weights(H, th, ty))
    k = np.arange(n)[:, None, None]
    v = img.astype(np.int64)
    acc = (lut[k, y1, x1, v] * (256 - wx) * (256 - wy) + lut[k, y1, x2, v] * wx * (256 - wy)
           + lut[k, y2, x1, v] * (256 - wx) * wy + lut[k, y2, x2, v] * wx * wy + 32768) >> 16
    out = acc.astype(np.uint8)
    return out[0] if squeeze else out


def clahe(img, tx, ty, clip):
    img = np.asarray(img)
    return apply(img, luts(img, tx, ty, clip), tx, ty)


def clahe_float(img, tx, ty, clip):
    """The textbook / OpenCV formula in float32: lutScale = 255 / T, round to nearest even, bilinear weights x / tw - 0.5
    between the tile centres.  The histogram, the clip and the redistribution are integers there too."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    img = img[None] if squeeze else img
    n, H, W = img.shape
    tw, th = tile_size(H, W, tx, ty)
    c = np.cumsum(clip_histograms(tile_histograms(img, tx, ty), int(clip)), axis=-1)
    scale = np.float32(255.0) / np.float32(tw * th)
    lut = np.clip(np.rint(c.astype(np.float32) * scale), 0, 255).astype(np.float32)

    def axis(m, t, tiles):
        f = np.arange(m, dtype=np.float32) / np.float32(t) - np.float32(0.5)
        i1 = np.floor(f).astype(np.int64)
        return np.clip(i1, 0, tiles - 1), np.clip(i1 + 1, 0, tiles - 1), (f - i1.astype(np.float32)).astype(np.float32)

    x1, x2, xa = (v[None, None, :] for v in axis(W, tw, tx))
    y1, y2, ya = (v[None, :, None] for v in axis(H, th, ty))
    k = np.arange(n)[:, None, None]
    one = np.float32(1.0)
    res = ((lut[k, y1, x1, img] * (one - xa) + lut[k, y1, x2, img] * xa) * (one - ya)
           + (lut[k, y2, x1, img] * (one - xa) + lut[k, y2, x2, img] * xa) * ya)
    assert res.dtype == np.float32
    out = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    return out[0] if squeeze else out


def murk(frames, t0=0.08, s=0.25, A=150):
    """Turbid water with the vehicle's own lamp: transmission t = t0 exp(-r^2 / (2 s^2)) falls off from the image centre
    (r in units of the image WIDTH on both axes), the rest is veiling light A.  frames uint8 [..., H, W] -> uint8."""
    frames = np.asarray(frames)
    H, W = frames.shape[-2:]
    x = (np.arange(W, dtype=np.float64) - (W - 1) / 2.0) / W
    y = (np.arange(H, dtype=np.float64) - (H - 1) / 2.0) / W
    r2 = x[None, :] ** 2 + y[:, None] ** 2
    t = t0 * np.exp(-r2 / (2.0 * s * s))
    return np.floor(frames.astype(np.float64) * t + A * (1.0 - t) + 0.5).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# images of the kernel tests


def image_kinds(n, H, W, seed=0):
    """name -> uint8 [n, H, W]: the image kinds the contract was checked on."""
    rng = np.random.default_rng(seed)
    ramp = ((np.arange(W)[None, :] * 3 + np.arange(H)[:, None] * 5) % 256).astype(np.uint8)
    two = np.where((np.arange(W)[None, :] // 7 + np.arange(H)[:, None] // 5) % 2 == 0, 40, 200).astype(np.uint8)
    uniform = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    return {"uniform": uniform, "zeros": np.zeros((n, H, W), np.uint8), "grey128": np.full((n, H, W), 128, np.uint8),
            "white": np.full((n, H, W), 255, np.uint8), "narrow": rng.integers(140, 150, (n, H, W), dtype=np.uint8),
            "ramp": np.stack([np.roll(ramp, 3 * i, axis=1) for i in range(n)]),
            "two_level": np.stack([np.roll(two, 2 * i, axis=0) for i in range(n)]), "murky": murk(uniform)}
