"""vus_orient_rbrief_tiled where its patch loaders read whole 16-byte block rows (csrc/orient.hip: TiledDiscPair,
TiledBriefRegs): bit for bit against the numpy statement of tests/orb_ref.py, with and without `order`, and against the
row-major entry point on the same planes.

What the loaders can get wrong, and the case that holds it:
  * the window of a keypoint starts at the 16-byte boundary below x - radius, so there are 16 byte alignments
    a = (x - radius) & 15 and 8 row phases (y - radius) & 7; the descriptor window is three pieces wide for a <= 11 and
    four beyond -- every pixel of 56 x 96 noise planes is a keypoint (96 is the smallest width with both forms inside the
    image), and of 40 x 64 planes, where a four-piece window fits only as the whole width;
  * a window that leaves the image takes the replicate-clamped path: keypoints whose window ends exactly at, and one
    pixel past, each image edge, for both patches;
  * the centroid patches of two keypoints share three loads, the second may be missing: live counts 0 .. 8 per wave;
  * weights and rotated offsets at every alignment: single-pixel planes and their complements;
  * the bytes of a piece that lie outside the disc or the 37 x 37 window: a patch of one value inside another.
The cases are generated once per module and not modified."""
import numpy as np
import pytest

import orb_ref as R
from test_orient_adversarial_gpu import _dev, gpu_order, run_entry
from visual_underwater_slam_amd.frontend import tile_planes

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, make):
    """(img, blur, keys, counts, H, W, ref) of a named case, generated and referenced once."""
    if name not in _CASES:
        img, blur, keys, counts, H, W = make()
        ref = R.orient_rbrief(img, blur, keys, counts, H, W)
        for a in (img, blur, keys, counts, *ref.values()):
            a.setflags(write=False)
        _CASES[name] = (img, blur, keys, counts, H, W, ref)
    return _CASES[name]


def check(case):
    """Tiled with the cell order, tiled without an order and row-major: all equal to the reference."""
    img, blur, keys, counts, H, W, ref = case
    n, max_kp = keys.shape
    assert W % 16 == 0 and H % 8 == 0
    img_d, blur_d, keys_d, counts_d = _dev(img), _dev(blur), _dev(keys.view(np.int32)), _dev(counts)
    _, cell_d = gpu_order(keys_d, counts_d, n, max_kp, H, W)
    img_t, blur_t = tile_planes(img_d), tile_planes(blur_d)
    for entry, a, b, order_d in (("tiled", img_t, blur_t, cell_d), ("tiled", img_t, blur_t, None), ("plain", img_d, blur_d, None)):
        desc, ang = run_entry(entry, a, b, keys_d, counts_d, order_d, n, H, W, W, max_kp)
        tag = (entry, "ordered" if order_d is not None else "unordered")
        bad_a = np.argwhere(ang != ref["angle"])
        assert bad_a.size == 0, (tag, "angle", len(bad_a), bad_a[:5].tolist())
        bad_d = np.argwhere((desc != ref["desc"]).any(-1))
        assert bad_d.size == 0, (tag, "descriptor", len(bad_d), bad_d[:5].tolist())
    return ref


def window(y, x, W, radius, brief):
    """Per keypoint: first row, last row, first column and one past the last column of the window its loader reads."""
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    xa = (x - radius) & ~np.int64(15)
    pieces = np.where(((x - radius) & 15) <= 11, 3, 4) if brief else 3
    return y - radius, y + radius, xa, xa + 16 * pieces


def inside(y, x, H, W, radius, brief):
    y0, y1, x0, x1 = window(y, x, W, radius, brief)
    return (y0 >= 0) & (y1 < H) & (x0 >= 0) & (x1 <= W)


# ---- every pixel a keypoint
def _every_pixel(H, W):
    def make():
        img, blur, keys, counts, _ = R.every_pixel_case(H, W, W, shuffle=True, seed=21)
        return img, blur, keys, counts, H, W
    return make


def test_every_pixel_56x96_has_every_alignment_row_phase_and_form(gpu):
    case = _case("every:56x96", _every_pixel(56, 96))
    keys, H, W = case[2], case[4], case[5]
    pos = keys[0].astype(np.int64) & R.KEY_POS_MASK
    y, x = pos // W, pos % W
    for radius, brief in ((R.RADIUS, False), (R.REACH, True)):
        fast = inside(y, x, H, W, radius, brief)
        assert fast.any() and (~fast).any()
        assert set(((x - radius) & 15)[fast]) == set(range(16))            # both descriptor forms among them
        assert {(int(a), int(p)) for a, p in zip(((x - radius) & 15)[fast], ((y - radius) & 7)[fast])} >= \
            {(a, p) for a in range(16) for p in range(min(8, H - 2 * radius))}
    check(case)


def test_every_pixel_40x64_where_a_four_piece_window_is_the_whole_width(gpu):
    """Three-piece windows fit at two starts; a four-piece window only at column 0, where it ends exactly at W."""
    case = _case("every:40x64", _every_pixel(40, 64))
    keys, H, W = case[2], case[4], case[5]
    pos = keys[0].astype(np.int64) & R.KEY_POS_MASK
    y, x = pos // W, pos % W
    fast = inside(y, x, H, W, R.REACH, True)
    four = ((x - R.REACH) & 15) > 11
    assert (fast & ~four).any() and (fast & four).any() and (x[fast & four] - R.REACH < 16).all()
    assert (~fast[four & (x - R.REACH >= 16)]).all() and (four & (x - R.REACH >= 16)).any()
    check(case)


# ---- the boundary between the fast and the clamped path
EDGE_H, EDGE_W = 64, 128


def _edges():
    rng = np.random.default_rng(22)
    H, W = EDGE_H, EDGE_W
    ys, xs = [], []
    for radius in (R.RADIUS, R.REACH):
        for y in (radius - 1, radius, H - 1 - radius, H - radius):        # top and bottom: one past, exactly at
            ys += [y] * W
            xs += list(range(W))
        for y in (radius, 29, 33, H - 1 - radius):                        # left and right: every column
            ys += [y] * W
            xs += list(range(W))
    keys = R.make_keys(rng, ys, xs, W)[None]
    img = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    return img, blur, keys, np.array([keys.shape[1]], np.int32), H, W


def test_windows_that_end_at_and_one_pixel_past_each_image_edge(gpu):
    case = _case("edges", _edges)
    keys, H, W = case[2], case[4], case[5]
    pos = keys[0].astype(np.int64) & R.KEY_POS_MASK
    y, x = pos // W, pos % W
    for radius, brief in ((R.RADIUS, False), (R.REACH, True)):
        y0, y1, x0, x1 = window(y, x, W, radius, brief)
        rows_in, cols_in = (y0 >= 0) & (y1 < H), (x0 >= 0) & (x1 <= W)
        # with the other direction inside: the window's first row at 0 and at -1, its last row at H - 1 and at H
        for v in (0, -1):
            assert ((y0 == v) & cols_in).any()
        for v in (H - 1, H):
            assert ((y1 == v) & cols_in).any()
        # its first column at 0 and left of it: x - radius = 0 and -1; its end at W, and the next keypoint whose end is past W
        assert ((x - radius == 0) & rows_in).any() and ((x - radius == -1) & rows_in).any()
        for form_pieces in ((3, 4) if brief else (3,)):                   # its end at W and one piece past it, per form
            sel = rows_in & (x1 - x0 == 16 * form_pieces)
            assert (sel & (x1 == W)).any() and (sel & (x1 == W + 16)).any()
        fits = {(int(a), int(b)) for a, b in zip(y[rows_in & cols_in], x[rows_in & cols_in])}
        past = {(int(a), int(b)) for a, b in zip(y[rows_in & (x1 > W)], x[rows_in & (x1 > W)])}
        assert any((a, b + 1) in past for a, b in fits)                   # one pixel further right and the window has left
    check(case)


# ---- live counts per wave
COUNT_SETS = {"0_to_8": ([0, 1, 2, 3, 4, 5, 6, 7, 8], 37), "second_and_later_waves": ([9, 11, 13, 15, 17, 0, 33, 36, 37], 37),
              "max_kp_13": ([13, 12, 11, 3, 0, 9, 10, 5, 13], 13)}


def _counts(name):
    def make():
        counts, max_kp = COUNT_SETS[name]
        rng = np.random.default_rng(23 + max_kp + len(name))
        H, W, n = 64, 96, len(counts)
        img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        blur = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        # two of three keypoints well inside (the paired fast path with a missing partner), the rest anywhere
        inner = rng.random((n, max_kp)) < 0.67
        ys = np.where(inner, rng.integers(18, H - 18, (n, max_kp)), rng.integers(0, H, (n, max_kp)))
        xs = np.where(inner, rng.integers(18, W - 46, (n, max_kp)), rng.integers(0, W, (n, max_kp)))
        keys = R.make_keys(rng, ys, xs, W)
        for i, c in enumerate(counts):
            keys[i, c:] = R.KEY_INVALID
        return img, blur, keys, np.array(counts, np.int32), H, W
    return make


@pytest.mark.parametrize("name", list(COUNT_SETS))
def test_live_counts_per_wave_over_nine_images(gpu, name):
    """Odd counts leave the second keypoint of a pair missing; max_kp is no multiple of 8 or 32; a count of 0; nine
    images wrap the block map's eight lanes."""
    counts, max_kp = COUNT_SETS[name]
    assert len(counts) == 9 and max_kp % 8 != 0 and 0 in counts and any(c % 2 for c in counts)
    if name == "0_to_8":
        assert sorted(counts) == list(range(9))
    ref = check(_case("counts:" + name, _counts(name)))
    for i, c in enumerate(counts):
        assert not ref["desc"][i, c:].any() and not ref["angle"][i, c:].any()


# ---- single-pixel planes
IMP_XS = 19 + 39 * np.arange(16)                   # (x - 18) & 15 = (1 + 7 j) & 15, (x - 15) & 15 = (4 + 7 j) & 15: all 16 each
IMP_YS = 19 + np.arange(16) % 8                    # rows 19 .. 26: every row phase of both patches


_IMP_OFFSETS = {False: {}, True: {}}                # [complement][bin] -> the offsets (dx, dy) of the bin's keypoints


def _blur_impulses(complement):
    def make():
        rng = np.random.default_rng(24 + int(complement))
        H, W, K = 48, 640, len(IMP_XS)
        img = rng.integers(0, 256, (R.N_BINS, H, W), dtype=np.uint8)
        blur = np.full((R.N_BINS, H, W), 255 if complement else 0, np.uint8)
        keys = np.zeros((R.N_BINS, K), np.uint32)
        d = np.arange(1, R.RADIUS + 1)
        for k in range(R.N_BINS):
            m10, m01 = R.sweep_moments(k)
            offs = _IMP_OFFSETS[complement][k] = R.impulse_offsets(k, complement, rng)[:K]
            for y, x, (ox, oy) in zip(IMP_YS, IMP_XS, offs):
                img[k, y + R.DISC_DY, x + R.DISC_DX] = 0
                if m10:
                    img[k, y, x + int(np.sign(m10)) * d] = R._axis_values(abs(m10))[1:]
                if m01:
                    img[k, y + int(np.sign(m01)) * d, x] = R._axis_values(abs(m01))[1:]
                blur[k, y + oy, x + ox] = 0 if complement else 255
            keys[k] = R.make_keys(rng, IMP_YS, IMP_XS, W)
        return img, blur, keys, np.full(R.N_BINS, K, np.int32), H, W
    return make




@pytest.mark.parametrize("complement", [False, True])
def test_one_smoothed_pixel_per_keypoint_at_every_alignment_and_bin(gpu, complement):
    """Image k serves bin k with one keypoint per byte alignment; the smoothed plane holds one pixel of 255 on 0 (or of 0
    on 255) per keypoint, at an offset out of the bin's rotated table, the farthest in each direction among them.  The
    expected words follow from the table alone."""
    assert set((IMP_XS - R.REACH) & 15) == set(range(16)) and set((IMP_XS - R.RADIUS) & 15) == set(range(16))
    assert set((IMP_YS - R.REACH) & 7) == set(range(8)) and set((IMP_YS - R.RADIUS) & 7) == set(range(8))
    case = _case(f"blur_impulse:{complement}", _blur_impulses(complement))
    ref = check(case)
    assert (ref["angle"] == np.arange(R.N_BINS, dtype=np.uint8)[:, None]).all()
    for k in range(R.N_BINS):
        want = R.pack_bits(np.stack([R.impulse_expected_bits(k, o, complement) for o in _IMP_OFFSETS[complement][k]]))
        assert np.array_equal(ref["desc"][k], want), k


def _image_impulses(complement):
    def make():
        rng = np.random.default_rng(26 + int(complement))
        H, W, n = 56, 96, 16
        img = np.full((n, H, W), 255 if complement else 0, np.uint8)
        py, px = 27, 40 + np.arange(n)                                    # the pixel walks through 16 columns
        img[np.arange(n), py, px] = 0 if complement else 255
        blur = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        dy, dx = [a.reshape(-1) for a in np.mgrid[-17:18, -17:18]]        # every disc offset and a rim outside the disc
        ys, xs = np.broadcast_to(py - dy, (n, dy.size)), px[:, None] - dx[None, :]
        keys = R.make_keys(rng, ys, xs, W)
        return img, blur, keys, np.full(n, dy.size, np.int32), H, W
    return make


@pytest.mark.parametrize("complement", [False, True])
def test_one_image_pixel_seen_from_every_disc_offset_at_every_alignment(gpu, complement):
    """One pixel of 255 on 0 (or 0 on 255) in the image plane, every position from which the disc sees it -- and a rim
    from which it must not -- a keypoint, with the pixel in 16 consecutive columns: each weight of the disc at each byte
    alignment decides a moment on its own."""
    case = _case(f"image_impulse:{complement}", _image_impulses(complement))
    keys, W, ref = case[2], case[5], case[6]
    x = (keys.astype(np.int64) & R.KEY_POS_MASK) % W
    px = 40 + np.arange(16)
    dx = px[:, None] - x
    for off in np.unique(dx):
        assert set(((x - R.RADIUS) & 15)[dx == off]) == set(range(16))
    if not complement:                                                    # outside the disc the pixel weighs nothing
        y = (keys.astype(np.int64) & R.KEY_POS_MASK) // W
        seen = np.abs(dx) <= R.HALF_WIDTH[np.minimum(np.abs(27 - y), R.RADIUS)]
        seen &= np.abs(27 - y) <= R.RADIUS
        assert ((ref["m10"] != 0) | (ref["m01"] != 0) | (dx == 0) & (y == 27))[seen].all()
        assert ((ref["m10"] == 0) & (ref["m01"] == 0))[~seen].all()
    check(case)


# ---- pad bytes
def _islands(inner, outer):
    def make():
        rng = np.random.default_rng(28)
        xs1, ys1 = 24 + 49 * np.arange(16), 24 + 41 * np.arange(8)        # (x - r) & 15 and (y - r) & 7 take every value
        H, W = 336, 800
        img = np.full((1, H, W), outer, np.uint8)
        blur = np.full((1, H, W), outer, np.uint8)
        ys, xs = [a.reshape(-1) for a in np.meshgrid(ys1, xs1, indexing="ij")]
        for y, x in zip(ys, xs):
            img[0, y + R.DISC_DY, x + R.DISC_DX] = inner
            blur[0, y - R.REACH:y + R.REACH + 1, x - R.REACH:x + R.REACH + 1] = inner
        keys = R.make_keys(rng, ys, xs, W)[None]
        return img, blur, keys, np.array([len(ys)], np.int32), H, W
    return make


@pytest.mark.parametrize("inner,outer", [(60, 200), (200, 60)])
def test_bytes_of_a_piece_outside_the_patch_do_not_leak(gpu, inner, outer):
    """The disc of the image and the 37 x 37 window of the smoothed plane hold one value, everything around them another:
    the moments are 0 by symmetry (bin 0) and every test compares equal bytes (all bits 0) unless a byte from outside the
    patch is weighed or tested.  16 alignments x 8 row phases."""
    xs1, ys1 = 24 + 49 * np.arange(16), 24 + 41 * np.arange(8)
    for r in (R.RADIUS, R.REACH):
        assert set((xs1 - r) & 15) == set(range(16)) and set((ys1 - r) & 7) == set(range(8))
    ref = check(_case(f"islands:{inner}:{outer}", _islands(inner, outer)))
    assert not ref["angle"].any() and not ref["desc"].any()
    assert not ref["m10"].any() and not ref["m01"].any()
