"""Plain numpy statement of intensity-centroid orientation + rotated BRIEF (include/vus.h: vus_orient_rbrief), written
from the header's definitions and the paper's (Rublee et al. 2011, sec. 4) and not from the oracle's loops, plus the
deterministic adversarial cases for it.  Test infrastructure only (a plain module, not a conftest).

The statement: the disc has radius 15 and the half-widths per row of include/vus_orb_tables.h; m10 = sum dx I and
m01 = sum dy I over the disc of `img` (its own pitch, coordinates replicate-clamped); the bin is the first maximum of
m10 cos_q14[k] + m01 sin_q14[k]; bit t of the descriptor is blur[p0] < blur[p1] at the bin's rotated test pair t
(blur pitch W, coordinates replicate-clamped), bit b of word w = test 64 w + b.  Slots at or beyond
min(max(kp_count, 0), max_kp) are all zero; the top 8 key bits are ignored.  All int64, vectorised over keypoints.

Every generator is seeded and returns (img [n, H, pitch] u8, blur [n, H, W] u8, keys [n, max_kp] u32, counts [n] i32,
meta)."""
import math
import os
import re

import numpy as np

N_BINS = 30
RADIUS = 15
REACH = 18                         # VUS_RBRIEF_REACH: max |offset| of a rotated test point
KEY_POS_MASK = 0x00FFFFFF
KEY_INVALID = 0xFFFFFFFF
CELL = 64                          # vus_orient_order groups by 64 x 64-pixel cell
MAX_CELLS = 1024

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_array(name):
    """An integer table of include/vus_orb_tables.h, read as tests/test_frontend_oracle.py reads them."""
    txt = open(os.path.join(_ROOT, "include", "vus_orb_tables.h")).read()
    m = re.search(name + r"\[[^\]]*\] = \{(.*?)\};", txt, re.S)
    return np.array([int(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()], np.int64)


def _half_widths():
    dx, dy = header_array("VUS_DISC_DX"), header_array("VUS_DISC_DY")
    return np.array([dx[np.abs(dy) == r].max() for r in range(RADIUS + 1)], np.int64)


# the disc: rows dy = -15 .. 15, columns -HALF_WIDTH[|dy|] .. HALF_WIDTH[|dy|], raster order
HALF_WIDTH = _half_widths()
DISC_DY = np.concatenate([np.full(2 * HALF_WIDTH[abs(r)] + 1, r) for r in range(-RADIUS, RADIUS + 1)]).astype(np.int64)
DISC_DX = np.concatenate([np.arange(-HALF_WIDTH[abs(r)], HALF_WIDTH[abs(r)] + 1) for r in range(-RADIUS, RADIUS + 1)]).astype(np.int64)

_THETA = 2.0 * np.pi * np.arange(N_BINS) / N_BINS
COS_Q14 = np.rint(np.cos(_THETA) * 16384).astype(np.int64)
SIN_Q14 = np.rint(np.sin(_THETA) * 16384).astype(np.int64)

BASE = header_array("VUS_RBRIEF_BASE").reshape(256, 4)     # (x0, y0, x1, y1) of the 256 learned pairs


def _rotated_pattern():
    c, s = np.cos(_THETA)[:, None], np.sin(_THETA)[:, None]
    rot = np.empty((N_BINS, 256, 4), np.int64)
    for h in (0, 2):
        x, y = BASE[None, :, h].astype(np.float64), BASE[None, :, h + 1].astype(np.float64)
        rot[:, :, h] = np.rint(x * c - y * s)              # np.rint: half to even
        rot[:, :, h + 1] = np.rint(x * s + y * c)
    return rot


ROT = _rotated_pattern()                                   # [bin, test, (x0, y0, x1, y1)]


def live_count(count, max_kp):
    return min(max(int(count), 0), int(max_kp))


def moments(plane, H, W, y, x):
    """(m10, m01) int64 of the keypoints (y, x) on one image plane [H, pitch]."""
    yy = np.clip(y[:, None] + DISC_DY[None, :], 0, H - 1)
    xx = np.clip(x[:, None] + DISC_DX[None, :], 0, W - 1)
    v = plane[yy, xx].astype(np.int64)
    return (v * DISC_DX).sum(1), (v * DISC_DY).sum(1)


def projections(m10, m01):
    return np.asarray(m10, np.int64)[..., None] * COS_Q14 + np.asarray(m01, np.int64)[..., None] * SIN_Q14


def descriptor_bits(plane, H, W, y, x, bins):
    """bool [k, 256] of the keypoints (y, x) with orientation bins `bins` on one smoothed plane [H, W]."""
    pat = ROT[bins]
    a = plane[np.clip(y[:, None] + pat[:, :, 1], 0, H - 1), np.clip(x[:, None] + pat[:, :, 0], 0, W - 1)]
    b = plane[np.clip(y[:, None] + pat[:, :, 3], 0, H - 1), np.clip(x[:, None] + pat[:, :, 2], 0, W - 1)]
    return a < b


def pack_bits(bits):
    """bool [k, 256] -> uint64 [k, 4], bit b of word w = test 64 w + b."""
    k = bits.shape[0]
    return np.packbits(bits.reshape(k, 4, 64), axis=-1, bitorder="little").view("<u8").reshape(k, 4).astype(np.uint64)


def orient_rbrief(img, blur, keys, counts, H, W):
    """The stage on img [n, H, pitch], blur [n, H, W]: dict(desc u64 [n, max_kp, 4], angle u8 [n, max_kp], and the
    intermediate m10, m01 i64 [n, max_kp] (0 in unused slots))."""
    n, max_kp = keys.shape
    assert img.shape[:2] == (n, H) and img.shape[2] >= W and blur.shape == (n, H, W)
    out = dict(desc=np.zeros((n, max_kp, 4), np.uint64), angle=np.zeros((n, max_kp), np.uint8),
               m10=np.zeros((n, max_kp), np.int64), m01=np.zeros((n, max_kp), np.int64))
    for i in range(n):
        c = live_count(counts[i], max_kp)
        if c == 0:
            continue
        pos = (keys[i, :c].astype(np.int64) & KEY_POS_MASK)
        y, x = pos // W, pos % W
        m10, m01 = moments(img[i], H, W, y, x)
        bins = np.argmax(projections(m10, m01), axis=1)    # np.argmax: the first maximum
        out["m10"][i, :c], out["m01"][i, :c], out["angle"][i, :c] = m10, m01, bins
        out["desc"][i, :c] = pack_bits(descriptor_bits(blur[i], H, W, y, x, bins))
    return out


def reference_order_is_valid(order, keys, counts, H, W):
    """vus_orient_order's contract: per image a permutation of [0, count) grouped by 64 x 64 cell in raster order, the
    identity beyond the count."""
    n, max_kp = keys.shape
    order = np.asarray(order)
    if order.shape != (n, max_kp):
        return False
    cw = (W + CELL - 1) // CELL
    for i in range(n):
        c = live_count(counts[i], max_kp)
        o = order[i].astype(np.int64)
        if not np.array_equal(np.sort(o[:c]), np.arange(c)) or not np.array_equal(o[c:], np.arange(c, max_kp)):
            return False
        pos = keys[i, o[:c]].astype(np.int64) & KEY_POS_MASK
        cell = (pos // W // CELL) * cw + (pos % W) // CELL
        if np.any(np.diff(cell) < 0):
            return False
    return True


def make_keys(rng, y, x, W):
    """Keys of the positions with arbitrary top 8 bits (the response byte: ignored by this stage)."""
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    return ((rng.integers(0, 256, y.shape).astype(np.int64) << 24) | (y * W + x)).astype(np.uint32)


# ---- the fast path of the kernel's patch loaders: (radius, row dwords, start alignment) per plane layout
LOADERS = {"row_major": ((15, 10, 4), (18, 10, 4)), "exact": ((15, 10, 1), (18, 10, 1)), "tiled": ((15, 10, 8), (18, 12, 8))}


def fast_path_conditions(y, x, H, W, loader):
    """bool [4, k]: y - R >= 0, y + R < H, xa >= 0, xa + 4 DW <= W with xa = x - R aligned down."""
    R, DW, align = loader
    xa = (np.asarray(x, np.int64) - R) & ~np.int64(align - 1)
    y = np.asarray(y, np.int64)
    return np.stack([y - R >= 0, y + R < H, xa >= 0, xa + 4 * DW <= W])


# ---- moments_case: prescribed (m10, m01)
MOMENT_AXIS_MAX = 255 * (RADIUS * (RADIUS + 1) // 2)       # 30600: what the keypoint's row (or column) alone can reach


def _axis_values(m):
    """v[1..15] in 0..255 with sum d v[d] == m (0 <= m <= 30600), largest distances first."""
    assert 0 <= m <= MOMENT_AXIS_MAX
    v = np.zeros(RADIUS + 1, np.int64)
    for d in range(RADIUS, 0, -1):
        v[d] = min(255, m // d)
        m -= v[d] * d
    assert m == 0
    return v


def tie_moments(k):
    """The smallest integer (m10, m01) whose projections on bins k and k + 1 (mod 30) are equal and positive."""
    k2 = (k + 1) % N_BINS
    dc, ds = int(COS_Q14[k] - COS_Q14[k2]), int(SIN_Q14[k] - SIN_Q14[k2])
    g = math.gcd(abs(dc), abs(ds))
    m = (-ds // g, dc // g)
    if m[0] * COS_Q14[k] + m[1] * SIN_Q14[k] < 0:
        m = (-m[0], -m[1])
    return int(m[0]), int(m[1])


def tie_step(k):
    """The unit step (along one axis) that turns the tie of bins k / k + 1 towards bin k + 1."""
    k2 = (k + 1) % N_BINS
    tc, ts = int(COS_Q14[k2] - COS_Q14[k]), int(SIN_Q14[k2] - SIN_Q14[k])
    return (int(np.sign(tc)), 0) if abs(tc) >= abs(ts) else (0, int(np.sign(ts)))


def sweep_moments(k, scale=3000):
    return int(np.rint(scale * np.cos(_THETA[k]))), int(np.rint(scale * np.sin(_THETA[k])))


MOM_CW, MOM_CH, MOM_X0, MOM_Y0 = 33, 32, 18, 16            # 33: consecutive keypoints walk through every byte alignment


def _moments_layout(n, cols):
    rows = (n + cols - 1) // cols
    W = -(-(MOM_X0 + MOM_CW * (cols - 1) + RADIUS + 1) // 16) * 16
    H = -(-(MOM_Y0 + MOM_CH * (rows - 1) + RADIUS + 1) // 8) * 8
    j = np.arange(n)
    return H, W, MOM_Y0 + MOM_CH * (j // cols), MOM_X0 + MOM_CW * (j % cols)


def moments_image(specs, rng, cols=5):
    """One image [H, W] with one keypoint per spec (m10, m01, fill): inside the keypoint's disc everything is `fill`
    (0 unless stated) except pixels on its row (m10 alone) and column (m01 alone); noise beyond the discs."""
    H, W, ys, xs = _moments_layout(len(specs), cols)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    d = np.arange(1, RADIUS + 1)
    for (m10, m01, fill), y, x in zip(specs, ys, xs):
        img[y + DISC_DY, x + DISC_DX] = fill
        if m10:
            img[y, x + int(np.sign(m10)) * d] = _axis_values(abs(m10))[1:]
        if m01:
            img[y + int(np.sign(m01)) * d, x] = _axis_values(abs(m01))[1:]
    return img, ys, xs


def _tie_triples(scaled):
    """Per adjacent bin pair: one unit before the tie, the tie, one unit after.  scaled: the tie vector times the
    largest factor that keeps it reachable, where the unit steps land in bins k and k + 1 themselves (next to the
    smallest ties, such as (0, 1) of bins 7 / 8, a unit step turns the moment by several bins)."""
    specs, want = [], []
    for k in range(N_BINS):
        (a, b), (sa, sb) = tie_moments(k), tie_step(k)
        if scaled:
            f = (MOMENT_AXIS_MAX - 1) // max(abs(a), abs(b))
            a, b = f * a, f * b
        specs += [(a - sa, b - sb, 0), (a, b, 0), (a + sa, b + sb, 0)]
        want += [(k, "below"), (k, "tie"), (k, "above")]
    return specs, want


def _moment_specs(name):
    """(specs, roles, max_kp, count) of a named moments case."""
    if name == "ties":              # slots 3k, 3k + 1, 3k + 2: one unit before the tie of bins k / k + 1, the tie, one after
        specs, roles = _tie_triples(False)
        return specs, roles, len(specs) + 3, len(specs)
    if name == "ties_scaled":
        specs, roles = _tie_triples(True)
        return specs, roles, len(specs), len(specs)
    if name == "flat_axes_sweep":
        A = MOMENT_AXIS_MAX
        specs = [(0, 0, 0), (0, 0, 1), (0, 0, 255), (A, 0, 0), (0, A, 0), (-A, 0, 0), (0, -A, 0)]
        roles = [("flat", 0), ("flat", 1), ("flat", 255), ("axis", 0), ("axis", 1), ("axis", 2), ("axis", 3)]
        specs += [sweep_moments(k) + (0,) for k in range(N_BINS)]
        roles += [("sweep", k) for k in range(N_BINS)]
        return specs, roles, len(specs), len(specs)
    if name == "tie_slots":         # ties at slot 0, at slot 7 and alone in the third wave; the other live slots untied
        specs = [sweep_moments((7 * j) % N_BINS) + (0,) for j in range(17)]
        roles = [("sweep", (7 * j) % N_BINS) for j in range(17)]
        for slot, k in ((0, 3), (7, 29), (16, 7)):          # pairs 3/4, 29/0 and 7/8 straddle the kernel's lane groups
            specs[slot], roles[slot] = tie_moments(k) + (0,), (k, "tie")
        return specs, roles, 24, 17
    raise KeyError(name)


MOMENTS_CASES = ("ties", "ties_scaled", "flat_axes_sweep", "tie_slots")


def moments_case(name, seed=11):
    rng = np.random.default_rng(seed)
    specs, roles, max_kp, count = _moment_specs(name)
    img, ys, xs = moments_image(specs, rng)
    H, W = img.shape
    blur = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    keys = np.full((1, max_kp), KEY_INVALID, np.uint32)
    keys[0, :count] = make_keys(rng, ys, xs, W)
    meta = dict(H=H, W=W, pitch=W, specs=specs, roles=roles)
    return img[None], blur, keys, np.array([count], np.int32), meta


# ---- saturated_case
SAT_DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
SAT_CELL = 40


def saturated_case(seed=12):
    """Image 0: eight 40 x 40 cells, each 255 on one side of the line through its centre keypoint and 0 on the other
    (the eight directions of SAT_DIRS).  Image 1: 255 everywhere, keypoints in the corners, on the edges and inside."""
    rng = np.random.default_rng(seed)
    H, W = 2 * SAT_CELL, 4 * SAT_CELL
    img = np.zeros((2, H, W), np.uint8)
    gy, gx = np.mgrid[0:SAT_CELL, 0:SAT_CELL] - SAT_CELL // 2
    ys, xs = [], []
    for j, (ux, uy) in enumerate(SAT_DIRS):
        r, c = divmod(j, 4)
        img[0, r * SAT_CELL:(r + 1) * SAT_CELL, c * SAT_CELL:(c + 1) * SAT_CELL] = np.where(gx * ux + gy * uy > 0, 255, 0)
        ys.append(r * SAT_CELL + SAT_CELL // 2)
        xs.append(c * SAT_CELL + SAT_CELL // 2)
    img[1] = 255
    y1 = [0, 0, H - 1, H - 1, H // 2, 0, H // 2, 17]
    x1 = [0, W - 1, 0, W - 1, W // 2, W // 2, W - 1, 23]
    blur = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    keys = np.stack([make_keys(rng, ys, xs, W), make_keys(rng, y1, x1, W)])
    return img, blur, keys, np.array([8, 8], np.int32), dict(H=H, W=W, pitch=W, dirs=SAT_DIRS)


# ---- impulse_case
IMP_CELL, IMP_ROWS, IMP_COLS = 38, 4, 5
IMP_PER_BIN = IMP_ROWS * IMP_COLS


def impulse_offsets(k, complement, rng):
    """IMP_PER_BIN distinct offsets (dx, dy) out of bin k's rotated table -- second points, or first points for the
    complementary plane -- the ones of largest |dx| and |dy| in each direction first, the rest drawn."""
    pts = np.unique(ROT[k][:, 0:2] if complement else ROT[k][:, 2:4], axis=0)
    first = [pts[np.argmax(pts[:, 0])], pts[np.argmin(pts[:, 0])], pts[np.argmax(pts[:, 1])], pts[np.argmin(pts[:, 1])]]
    chosen = []
    for p in first + list(pts[rng.permutation(len(pts))]):
        if not any((p == q).all() for q in chosen):
            chosen.append(p)
        if len(chosen) == IMP_PER_BIN:
            break
    return np.array(chosen, np.int64)


def impulse_expected_bits(k, offset, complement):
    """From the table alone.  One pixel of 255 on 0: a < b exactly where the second point is the pixel and the first is
    not.  One pixel of 0 on 255: where the first point is the pixel and the second is not."""
    at0 = (ROT[k][:, 0:2] == offset).all(1)
    at1 = (ROT[k][:, 2:4] == offset).all(1)
    return (at0 & ~at1) if complement else (at1 & ~at0)


def impulse_case(complement=False, seed=13):
    """Image k serves bin k: IMP_PER_BIN keypoints in 38 x 38 cells, moments as in moments_case (the sweep), and a blur
    plane of 0 with one pixel of 255 per keypoint (complement: 255 with one pixel of 0).  meta['expected'] holds the
    descriptors the table dictates."""
    rng = np.random.default_rng(seed + int(complement))
    H, W = IMP_ROWS * IMP_CELL, -(-(IMP_COLS * IMP_CELL) // 16) * 16
    img = rng.integers(0, 256, (N_BINS, H, W), dtype=np.uint8)
    blur = np.full((N_BINS, H, W), 255 if complement else 0, np.uint8)
    keys = np.zeros((N_BINS, IMP_PER_BIN), np.uint32)
    expected = np.zeros((N_BINS, IMP_PER_BIN, 4), np.uint64)
    offsets = np.zeros((N_BINS, IMP_PER_BIN, 2), np.int64)
    j = np.arange(IMP_PER_BIN)
    ys, xs = IMP_CELL * (j // IMP_COLS) + IMP_CELL // 2, IMP_CELL * (j % IMP_COLS) + IMP_CELL // 2
    d = np.arange(1, RADIUS + 1)
    for k in range(N_BINS):
        m10, m01 = sweep_moments(k)
        offsets[k] = impulse_offsets(k, complement, rng)
        for y, x, (ox, oy) in zip(ys, xs, offsets[k]):
            img[k, y + DISC_DY, x + DISC_DX] = 0
            if m10:
                img[k, y, x + int(np.sign(m10)) * d] = _axis_values(abs(m10))[1:]
            if m01:
                img[k, y + int(np.sign(m01)) * d, x] = _axis_values(abs(m01))[1:]
            blur[k, y + oy, x + ox] = 0 if complement else 255
        expected[k] = pack_bits(np.stack([impulse_expected_bits(k, o, complement) for o in offsets[k]]))
        keys[k] = make_keys(rng, ys, xs, W)
    meta = dict(H=H, W=W, pitch=W, expected=expected, offsets=offsets)
    return img, blur, keys, np.full(N_BINS, IMP_PER_BIN, np.int32), meta


# ---- equal_planes_case
EQUAL_PLANES = ("const0", "const128", "const255", "checker1", "checker2", "xramp1", "yramp1", "xramp4", "yramp4")


def equal_planes_case(seed=14):
    """One image per smoothed plane of EQUAL_PLANES (constants: every bit 0; checkerboards and ramps: many exact
    equalities, and a different answer for an offset that is off by one), 260 keypoints each, the corners included."""
    rng = np.random.default_rng(seed)
    H, W, K = 48, 64, 260
    yy, xx = np.mgrid[0:H, 0:W]
    planes = dict(const0=0 * xx, const128=0 * xx + 128, const255=0 * xx + 255, checker1=((xx + yy) & 1) * 200 + 20,
                  checker2=(((xx >> 1) + (yy >> 1)) & 1) * 200 + 20, xramp1=xx, yramp1=yy, xramp4=xx >> 2, yramp4=yy >> 2)
    blur = np.stack([planes[p] for p in EQUAL_PLANES]).astype(np.uint8)
    n = len(EQUAL_PLANES)
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    ys, xs = rng.integers(0, H, (n, K)), rng.integers(0, W, (n, K))
    ys[:, :4], xs[:, :4] = [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]
    keys = make_keys(rng, ys, xs, W)
    return img, blur, keys, np.full(n, K, np.int32), dict(H=H, W=W, pitch=W, planes=EQUAL_PLANES)


# ---- every_pixel_case
EVERY_PIXEL_SHAPES = [(48, 64, 64), (40, 44, 44), (37, 40, 40), (31, 40, 40), (20, 20, 20), (41, 51, 51), (33, 47, 47),
                      (48, 64, 80), (48, 64, 67), (47, 64, 66), (40, 48, 48)]
EVERY_PIXEL_TILED_SHAPES = [(48, 64, 64), (40, 48, 48)]    # W % 16 == 0, H % 8 == 0, pitch == W: the tiled entry point too


def every_pixel_case(H, W, pitch, shuffle=False, seed=15):
    """Every pixel of a noise image is a keypoint (max_kp = H W), in raster order or in a seeded shuffle; the padding
    bytes of a pitch wider than W are noise too."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    img = rng.integers(0, 256, (1, H, pitch), dtype=np.uint8)
    blur = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    pos = np.arange(H * W)
    if shuffle:
        pos = rng.permutation(pos)
    keys = make_keys(rng, pos // W, pos % W, W)[None]
    return img, blur, keys, np.array([H * W], np.int32), dict(H=H, W=W, pitch=pitch)


# ---- counts_case
COUNTS_N_IMG = (1, 7, 8, 9, 17)
COUNTS_MAX_KP = (1, 8, 33, 100)


def count_choices(max_kp):
    return [-3, 0, 1, 7, 8, 9, 31, 32, 33, max_kp - 1, max_kp, max_kp + 5]


def counts_case(n_img, max_kp, seed=16):
    """n_img images of 64 x 96, per-image counts out of count_choices (all of them once n_img >= 12; below, a window
    that moves with the case), keypoints anywhere, unused slots VUS_KEY_INVALID."""
    rng = np.random.default_rng(seed + 100 * n_img + max_kp)
    H, W = 64, 96
    ch = count_choices(max_kp)
    start = COUNTS_N_IMG.index(n_img) * 5 + COUNTS_MAX_KP.index(max_kp) * 3
    counts = np.array([ch[(start + i) % len(ch)] for i in range(n_img)], np.int32)
    img = rng.integers(0, 256, (n_img, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (n_img, H, W), dtype=np.uint8)
    keys = make_keys(rng, rng.integers(0, H, (n_img, max_kp)), rng.integers(0, W, (n_img, max_kp)), W)
    for i in range(n_img):
        keys[i, live_count(counts[i], max_kp):] = KEY_INVALID
    return img, blur, keys, counts, dict(H=H, W=W, pitch=W)


# ---- order_case: keys only
ORDER_CASES = ("one_cell", "one_per_cell", "count0", "count_full", "small_max_kp", "max_kp_8192", "odd_width", "cells_1024",
               "cells_1056_refused")


def order_case(name, seed=17):
    """(None, None, keys, counts, meta) for vus_orient_order; meta['refused'] where the library must refuse the shape."""
    rng = np.random.default_rng(seed + ORDER_CASES.index(name))
    H, W, max_kp, refused = 192, 256, 300, False
    rand = lambda n, k: (rng.integers(0, H, (n, k)), rng.integers(0, W, (n, k)))
    if name == "one_cell":
        ys, xs = rng.integers(64, 128, (2, max_kp)), rng.integers(128, 192, (2, max_kp))
        counts = [max_kp, 77]
    elif name == "one_per_cell":
        max_kp = 12
        cy, cx = np.divmod(rng.permutation(12), 4)
        ys, xs = (64 * cy + rng.integers(0, 64, 12))[None], (64 * cx + rng.integers(0, 64, 12))[None]
        counts = [12]
    elif name == "count0":
        (ys, xs), counts = rand(2, max_kp), [0, 0]
    elif name == "count_full":
        (ys, xs), counts = rand(3, max_kp), [max_kp, max_kp, max_kp]
    elif name == "small_max_kp":
        max_kp = 37
        (ys, xs), counts = rand(3, max_kp), [37, 5, 36]
    elif name == "max_kp_8192":
        max_kp = 8192
        (ys, xs), counts = rand(2, max_kp), [8192, 5000]
    elif name == "odd_width":
        H, W = 100, 203
        (ys, xs), counts = rand(2, max_kp), [max_kp, 123]
    elif name == "cells_1024":
        H, W, max_kp = 2048, 2048, 2500
        (ys, xs), counts = rand(1, max_kp), [max_kp]
    elif name == "cells_1056_refused":
        H, W, max_kp, refused = 2048, 2049, 64, True
        (ys, xs), counts = rand(1, max_kp), [max_kp]
    else:
        raise KeyError(name)
    keys = make_keys(rng, ys, xs, W)
    return None, None, keys, np.array(counts, np.int32), dict(H=H, W=W, max_kp=max_kp, refused=refused)


# ---- the registry the CPU and the GPU tests share: every image case by name, generated and referenced once
def _every_pixel_names():
    return [f"every_pixel:{H}x{W}p{p}:{o}" for H, W, p in EVERY_PIXEL_SHAPES for o in ("raster", "shuffled")]


def image_case_names():
    return ([f"moments:{m}" for m in MOMENTS_CASES] + ["saturated", "impulse", "impulse_complement", "equal_planes"] +
            _every_pixel_names() + [f"counts:{n}:{k}" for n in COUNTS_N_IMG for k in COUNTS_MAX_KP])


_CACHE = {}


def image_case(name):
    """(img, blur, keys, counts, meta, ref) of a named case; ref = orient_rbrief(...) of it.  Cached: read-only."""
    if name not in _CACHE:
        kind, _, arg = name.partition(":")
        if kind == "moments":
            c = moments_case(arg)
        elif kind == "saturated":
            c = saturated_case()
        elif kind in ("impulse", "impulse_complement"):
            c = impulse_case(kind == "impulse_complement")
        elif kind == "equal_planes":
            c = equal_planes_case()
        elif kind == "every_pixel":
            shape, order = arg.split(":")
            H, W, p = (int(v) for v in re.match(r"(\d+)x(\d+)p(\d+)", shape).groups())
            c = every_pixel_case(H, W, p, order == "shuffled")
        elif kind == "counts":
            c = counts_case(*(int(v) for v in arg.split(":")))
        else:
            raise KeyError(name)
        img, blur, keys, counts, meta = c
        ref = orient_rbrief(img, blur, keys, counts, meta["H"], meta["W"])
        for a in (img, blur, keys, counts, *ref.values()):
            a.setflags(write=False)
        _CACHE[name] = (img, blur, keys, counts, meta, ref)
    return _CACHE[name]
