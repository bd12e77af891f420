"""vus_orient_rbrief_tiled where its loaders deal a patch's 16-byte pieces to the lanes (csrc/orient.hip: disc_piece,
brief_piece): bit for bit against the numpy statement of tests/orb_ref.py, with and without `order`.

A dealing is a map slot -> (row, piece column).  The loads, the LDS stores and the disc weights must all follow the same
map; tests/test_orient_block_rows_gpu.py and tests/test_orient_adversarial_gpu.py hold the alignments, the clamped path,
the live counts and the weights on noise and single pixels.  What only a dealing can get wrong, and the case that holds it:
  * a piece delivered to another piece's slot, or weighed with another piece's weights -- planes on which every 16-byte
    block row carries its own value, a hash of (y, x >> 4): any exchange of two pieces changes the bytes under the disc
    and under the tests.  One keypoint per byte alignment and row phase of both patches, all in the fast path;
  * the block-row step 8 W - 128 and the fields packed beside the piece's offset at the workload's width -- a 48 x 1280
    plane, keypoints in the first, a middle and the last block column at row phases 0, 1, 2 and 7, where a 31-row patch
    spans four and five block rows;
  * the second keypoint of a pair starting in the middle of a wave-load, or missing -- pairs in all four mixes of fast
    and clamped path, odd live counts whose last keypoint is a fast one and a clamped one;
  * the descriptor patch's last row and the dword column of the wide form -- a smoothed plane that is constant but for row
    y + 18 and columns x + 15 .. x + 18 of its keypoints.
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


def _yx(keys, W):
    pos = keys.astype(np.int64) & R.KEY_POS_MASK
    return pos // W, pos % W


def check(case):
    """The tiled entry point with the cell order and without an order: both equal to the reference."""
    img, blur, keys, counts, H, W, ref = case
    n, max_kp = keys.shape
    assert W % 16 == 0 and H % 8 == 0
    img_d, blur_d, keys_d, counts_d = _dev(img), _dev(blur), _dev(keys.view(np.int32)), _dev(counts)
    _, cell_d = gpu_order(keys_d, counts_d, n, max_kp, H, W)
    img_t, blur_t = tile_planes(img_d), tile_planes(blur_d)
    y, x = _yx(keys, W)
    for order_d in (cell_d, None):
        desc, ang = run_entry("tiled", img_t, blur_t, keys_d, counts_d, order_d, n, H, W, W, max_kp)
        tag = "ordered" if order_d is not None else "unordered"
        bad = np.argwhere(ang != ref["angle"])
        assert bad.size == 0, (tag, "angle", len(bad), [(i, k, int(y[i, k]), int(x[i, k])) for i, k in bad[:5].tolist()])
        bad = np.argwhere((desc != ref["desc"]).any(-1))
        assert bad.size == 0, (tag, "descriptor", len(bad), [(i, k, int(y[i, k]), int(x[i, k])) for i, k in bad[:5].tolist()])
    return ref


def fast(y, x, H, W, radius, brief):
    """Whether the loader reads the keypoint's window in its fast path: whole pieces from the 16-byte boundary below
    x - radius, three per row, four for the descriptor patch at alignments past 11."""
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    xa = (x - radius) & ~np.int64(15)
    pieces = np.where(((x - radius) & 15) <= 11, 3, 4) if brief else 3
    return (y - radius >= 0) & (y + radius < H) & (xa >= 0) & (xa + 16 * pieces <= W)


# ---- every block row its own value
HASH_H, HASH_W, HASH_N = 56, 96, 8


def _hash_plane(rng, n, H, W):
    """byte = a random function of (image, y, x >> 4): the 16 bytes of a block row are equal, no two block rows related"""
    return np.repeat(rng.integers(0, 256, (n, H, W // 16), dtype=np.uint8), 16, axis=2)


def _block_row_hash():
    rng = np.random.default_rng(91)
    H, W, n = HASH_H, HASH_W, HASH_N
    img, blur = _hash_plane(rng, n, H, W), _hash_plane(rng, n, H, W)
    a, p = [v.reshape(-1) for v in np.meshgrid(np.arange(16), np.arange(8), indexing="ij")]
    ys, xs = R.REACH + p, R.REACH + 16 + a            # the descriptor window starts at block column 1, row phase p
    keys = np.stack([R.make_keys(rng, ys, xs, W) for _ in range(n)])
    return img, blur, keys, np.full(n, len(ys), np.int32), H, W


def test_every_block_row_its_own_value_at_every_alignment_and_row_phase(gpu):
    case = _case("block_row_hash", _block_row_hash)
    img, blur, keys, H, W = case[0], case[1], case[2], case[4], case[5]
    for plane in (img, blur):
        assert (plane.reshape(HASH_N, H, W // 16, 16) == plane.reshape(HASH_N, H, W // 16, 16)[..., :1]).all()
    y, x = _yx(keys[0], W)
    every = {(a, p) for a in range(16) for p in range(8)}
    for radius, brief in ((R.RADIUS, False), (R.REACH, True)):
        assert fast(y, x, H, W, radius, brief).all()
        assert {(int(a), int(p)) for a, p in zip((x - radius) & 15, (y - radius) & 7)} == every
    ref = check(case)
    assert len(np.unique(ref["angle"])) > R.N_BINS // 2          # the planes do decide the angle


# ---- the workload's width
WIDE_H, WIDE_W = 48, 1280
WIDE_PHASES = (0, 1, 2, 7)


def _wide():
    rng = np.random.default_rng(92)
    H, W = WIDE_H, WIDE_W
    img = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    cols = list(range(R.RADIUS, R.RADIUS + 34)) + list(range(640, 656)) + list(range(W - 66, W - R.RADIUS))
    rows = sorted({r + p for r in (R.RADIUS, R.REACH) for p in WIDE_PHASES})
    ys, xs = [v.reshape(-1) for v in np.meshgrid(rows, cols, indexing="ij")]
    keys = R.make_keys(rng, ys, xs, W)[None]
    return img, blur, keys, np.array([keys.shape[1]], np.int32), H, W


def test_first_middle_and_last_block_column_of_a_1280_wide_plane(gpu):
    case = _case("wide", _wide)
    keys, H, W = case[2], case[4], case[5]
    y, x = _yx(keys[0], W)
    for radius, brief in ((R.RADIUS, False), (R.REACH, True)):
        ok = fast(y, x, H, W, radius, brief)
        xa, a, p = (x - radius) & ~np.int64(15), (x - radius) & 15, (y - radius) & 7
        end = xa + 16 * (np.where(a <= 11, 3, 4) if brief else 3)
        for where in (xa == 0, end == W, (xa > 512) & (end < 768)):
            for form in ((a <= 11, a > 11) if brief else (a >= 0,)):
                assert {int(v) for v in p[ok & where & form]} >= set(WIDE_PHASES), (radius, brief)
        assert (~ok).any()                                       # and windows that leave the plane at either end
    block_rows = lambda p: (p + 2 * R.RADIUS) // 8 + 1            # of a 31-row patch whose first row is p rows into a block
    assert {block_rows(p) for p in WIDE_PHASES} == {4, 5}
    check(case)


# ---- pairs
PAIR_H, PAIR_W, PAIR_MAX_KP = 40, 64, 32
PAIR_COUNTS = [29, 27, 31, 25]


def _pair_mix(i):
    """Keypoint i is the (i & 1)-th of pair i >> 1; the pairs run through (fast, fast), (fast, clamped), (clamped, fast),
    (clamped, clamped): whether keypoint i takes the fast path."""
    mix = (i >> 1) & 3
    return mix in ((0, 1) if i & 1 == 0 else (0, 2))


def _pairs():
    rng = np.random.default_rng(93)
    H, W, n = PAIR_H, PAIR_W, len(PAIR_COUNTS)
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    yy, xx = [v.reshape(-1) for v in np.mgrid[0:H, 0:W]]
    inside = fast(yy, xx, H, W, R.RADIUS, False)
    ys, xs = np.zeros((n, PAIR_MAX_KP), np.int64), np.zeros((n, PAIR_MAX_KP), np.int64)
    for i in range(n):
        for k in range(PAIR_MAX_KP):
            j = rng.choice(np.flatnonzero(inside if _pair_mix(k) else ~inside))
            ys[i, k], xs[i, k] = yy[j], xx[j]
    keys = R.make_keys(rng, ys, xs, W)
    for i, c in enumerate(PAIR_COUNTS):
        keys[i, c:] = R.KEY_INVALID
    return img, blur, keys, np.array(PAIR_COUNTS, np.int32), H, W


def test_pairs_in_all_four_mixes_of_fast_and_clamped_with_odd_live_counts(gpu):
    case = _case("pairs", _pairs)
    keys, counts, H, W = case[2], case[3], case[4], case[5]
    assert all(c % 2 == 1 for c in PAIR_COUNTS)
    for i, c in enumerate(counts):
        y, x = _yx(keys[i, :c], W)
        f = fast(y, x, H, W, R.RADIUS, False)
        assert [bool(v) for v in f] == [_pair_mix(k) for k in range(c)]
        mixes = {(bool(f[k]), bool(f[k + 1])) for k in range(0, c - 1, 2)}
        assert mixes == {(True, True), (True, False), (False, True), (False, False)}
    # the keypoint without a partner: a fast one and a clamped one
    assert {_pair_mix(c - 1) for c in PAIR_COUNTS} == {True, False}
    ref = check(case)
    for i, c in enumerate(PAIR_COUNTS):
        assert not ref["desc"][i, c:].any() and not ref["angle"][i, c:].any()


# ---- the descriptor patch's last row and the dword column
EDGE_H, EDGE_W, EDGE_FLAT = 56, 672, 128
EDGE_XS = 20 + 41 * np.arange(16)                  # (x - 18) & 15 = (2 + 9 j) & 15: all 16, windows 41 columns apart
# the bins whose rotated pattern has tests in row + 18 (few have) and in columns + 15 .. + 18
EDGE_BINS = [k for k in range(R.N_BINS) if ((R.ROT[k][:, 1] == R.REACH) | (R.ROT[k][:, 3] == R.REACH)).any()
             and ((R.ROT[k][:, 0] >= 15) | (R.ROT[k][:, 2] >= 15)).any()]


def _edge_bins(n):
    """[n, 16]: the bin of every keypoint, each image starting one further into EDGE_BINS"""
    return np.array([[EDGE_BINS[(i + j) % len(EDGE_BINS)] for j in range(len(EDGE_XS))] for i in range(n)])


def _last_row_and_column():
    rng = np.random.default_rng(94)
    H, W, n = EDGE_H, EDGE_W, 8
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    blur = np.full((n, H, W), EDGE_FLAT, np.uint8)
    ys = np.repeat(R.REACH + np.arange(n)[:, None], len(EDGE_XS), axis=1)      # image p: row phase p
    xs = np.repeat(EDGE_XS[None, :], n, axis=0)
    d = np.arange(1, R.RADIUS + 1)
    for i in range(n):
        for y, x, k in zip(ys[i], xs[i], _edge_bins(n)[i]):
            m10, m01 = R.sweep_moments(k)                                  # the image: a disc whose moments point into bin k
            img[i, y + R.DISC_DY, x + R.DISC_DX] = 0
            if m10:
                img[i, y, x + int(np.sign(m10)) * d] = R._axis_values(abs(m10))[1:]
            if m01:
                img[i, y + int(np.sign(m01)) * d, x] = R._axis_values(abs(m01))[1:]
            blur[i, y + R.REACH, x - R.REACH:x + R.REACH + 1] = rng.integers(0, 256, 2 * R.REACH + 1)
            blur[i, y - R.REACH:y + R.REACH + 1, x + 15:x + R.REACH + 1] = rng.integers(0, 256, (2 * R.REACH + 1, 4))
    keys = R.make_keys(rng, ys, xs, W)
    return img, blur, keys, np.full(n, len(EDGE_XS), np.int32), H, W


def test_last_descriptor_row_and_the_dword_column_decide_the_words(gpu):
    """Every test of the pattern that does not touch row y + 18 or columns x + 15 .. x + 18 compares equal bytes and gives 0:
    the words are what the last row (r = 36) and, at alignments past 11, the dword column deliver."""
    case = _case("last_row_and_column", _last_row_and_column)
    blur, keys, H, W, ref = case[1], case[2], case[4], case[5], case[6]
    y, x = _yx(keys, W)
    assert fast(y, x, H, W, R.REACH, True).all()
    assert set(((x - R.REACH) & 15).reshape(-1)) == set(range(16)) and set(((y - R.REACH) & 7).reshape(-1)) == set(range(8))
    assert (((x - R.REACH) & 15) > 11).any()
    inner = np.stack([[blur[i, yy - R.REACH:yy + R.REACH, xx - R.REACH:xx + 15] for yy, xx in zip(y[i], x[i])] for i in range(len(y))])
    assert (inner == EDGE_FLAT).all()                              # no window reaches into a neighbour's row or columns
    assert len(EDGE_BINS) >= 4 and (ref["angle"] == _edge_bins(len(y))).all()   # every keypoint has tests that reach both
    assert ref["desc"].any(-1).sum() > 0.9 * y.size                # ... and nearly every one a test that they decide as 1
    check(case)
