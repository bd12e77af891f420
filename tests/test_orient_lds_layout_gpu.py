"""vus_orient_rbrief_tiled where its LDS images decide the result (csrc/orient.hip): the disc weights in rows of 13
eight-byte entries, folded over the disc's middle row, and the descriptor patch in rows of 80 bytes.  Bit for bit
against the numpy statement of tests/orb_ref.py, with the cell order and without an order, on 64 x 128 tiled planes.

What a layout of this kind can get wrong, and the case that holds it:
  * a piece stored to or read from another row's bytes, at some alignment or row phase -- random planes, one keypoint for
    every pair of byte alignment and row phase of both patches, each as the first and as the second of a pair of keypoints,
    odd live counts;
  * a weight entry's mask edge or its count byte after folding (row r reads the entries of row 30 - r; the entry in front
    of a row is the previous row's pad) -- planes with a single non-zero pixel per keypoint: on the disc's edge,
    dx = +-umax(dy), where the angle is the bin of (dx, dy), and one pixel outside it, where the moments are zero and
    the angle is bin 0; every disc row, every byte alignment, the sides whose own bin is not 0;
  * a test offset built for another pitch -- smoothed planes on which any two bytes of a 37 x 52 window that are at most two
    rows apart differ, every bin (the pattern's rows and columns +-18 among them), alignments up to 11 and past 11;
  * the clamped path storing another shape than the fast one -- keypoints within 18 pixels of each image edge.
The cases are generated once per module and not modified."""
import numpy as np
import pytest

import orb_ref as R
from test_orient_lane_dealing_gpu import _case, _yx, check, fast

pytestmark = pytest.mark.gpu

H, W = 64, 128
SLOT_X = (18, 50, 82)            # three keypoints per image row, 32 columns apart: their discs (31 wide) do not meet;
                                 # + j < 16: the wide descriptor window of the last ends at column 128


# ---- case 1: every alignment and row phase, as first and as second of a pair
def _alignments_and_phases():
    rng = np.random.default_rng(101)
    n = 2
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    a, p = [v.reshape(-1) for v in np.meshgrid(np.arange(16), np.arange(8), indexing="ij")]
    ys, xs = R.REACH + p, R.REACH + 16 + a
    # image 0: the 128 keypoints and one more; image 1: one more in front -- every keypoint changes its place in its pair
    ys = np.stack([np.append(ys, 30), np.insert(ys, 0, 30)])
    xs = np.stack([np.append(xs, 60), np.insert(xs, 0, 60)])
    keys = R.make_keys(rng, ys, xs, W)
    return img, blur, keys, np.full(n, keys.shape[1], np.int32), H, W


def test_every_alignment_and_row_phase_as_first_and_second_of_a_pair(gpu):
    case = _case("lds_alignments", _alignments_and_phases)
    keys, counts = case[2], case[3]
    assert all(c % 2 == 1 for c in counts)
    every = {(a, p) for a in range(16) for p in range(8)}
    (y0, x0), (y1, x1) = _yx(keys[0], W), _yx(keys[1], W)
    # the keypoint at place k of image 0 is at place k + 1 of image 1: the first member of a pair in one, the second in the other
    assert np.array_equal(y0[:-1], y1[1:]) and np.array_equal(x0[:-1], x1[1:])
    for radius, brief in ((R.RADIUS, False), (R.REACH, True)):
        assert fast(y0, x0, H, W, radius, brief).all() and fast(y1, x1, H, W, radius, brief).all()
        assert {(int(a), int(p)) for a, p in zip((x0[:-1] - radius) & 15, (y0[:-1] - radius) & 7)} == every
    check(case)


# ---- case 2: one hot pixel per keypoint, on the disc's edge and just outside it
def _hot_specs():
    """(dy, dx, inside) of every disc row, both sides, the edge pixel and the one beyond it -- the sides whose edge pixel's own
    bin is not 0."""
    specs = []
    for dy in range(-R.RADIUS, R.RADIUS + 1):
        um = int(R.HALF_WIDTH[abs(dy)])
        for side in (-1, 1):
            if int(np.argmax(R.projections(side * um, dy))) == 0:
                continue
            specs += [(dy, side * um, True), (dy, side * (um + 1), False)]
    return specs


def _one_hot():
    rng = np.random.default_rng(102)
    specs = _hot_specs()
    per = len(SLOT_X)
    groups = [specs[s:s + per] for s in range(0, len(specs), per)]
    n = 16 * len(groups)
    img = np.zeros((n, H, W), np.uint8)
    blur = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    ys, xs = np.zeros((n, per), np.int64), np.zeros((n, per), np.int64)
    counts = np.zeros(n, np.int32)
    for j in range(16):
        for g, grp in enumerate(groups):
            i = j * len(groups) + g
            counts[i] = len(grp)
            for s, (dy, dx, _) in enumerate(grp):
                ys[i, s], xs[i, s] = R.REACH + (j & 7), SLOT_X[s] + j
                img[i, ys[i, s] + dy, xs[i, s] + dx] = rng.integers(1, 256)
    keys = R.make_keys(rng, ys, xs, W)
    for i, c in enumerate(counts):
        keys[i, c:] = R.KEY_INVALID
    return img, blur, keys, counts, H, W


def test_one_hot_pixel_on_the_disc_edge_and_one_pixel_outside_it(gpu):
    case = _case("lds_one_hot", _one_hot)
    img, keys, counts, ref = case[0], case[2], case[3], case[6]
    specs = _hot_specs()
    assert {dy for dy, _, _ in specs} == set(range(-R.RADIUS, R.RADIUS + 1))          # every disc row
    per, n_groups = len(SLOT_X), -(-len(specs) // len(SLOT_X))
    seen = set()
    for i in range(len(counts)):
        j, g = divmod(i, n_groups)
        y, x = _yx(keys[i, :counts[i]], W)
        assert fast(y, x, H, W, R.RADIUS, False).all()
        for s in range(counts[i]):
            dy, dx, inside = specs[g * per + s]
            assert img[i, y[s] + dy, x[s] + dx] != 0                                   # the hot pixel, alone on or beside its disc
            assert np.count_nonzero(img[i, y[s] + R.DISC_DY, x[s] + R.DISC_DX]) == int(inside)
            want = int(np.argmax(R.projections(dx, dy))) if inside else 0
            assert (want != 0) == inside and ref["angle"][i, s] == want
            seen.add((dy, dx, int((x[s] - R.RADIUS) & 15)))
    assert seen == {(dy, dx, a) for dy, dx, _ in specs for a in range(16)}            # ... at every byte alignment
    check(case)


# ---- case 3: a smoothed plane whose window bytes differ, every bin, narrow and wide
PAT_A, PAT_B, PAT_M = 89, 7, 251


def _pattern_plane():
    yy, xx = np.mgrid[0:H, 0:W]
    return ((PAT_A * yy + PAT_B * xx) % PAT_M).astype(np.uint8)


def _every_bin():
    rng = np.random.default_rng(103)
    per = len(SLOT_X)
    n = 16 * R.N_BINS // per
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    blur = np.repeat(_pattern_plane()[None], n, axis=0)
    ys, xs = np.zeros((n, per), np.int64), np.zeros((n, per), np.int64)
    d = np.arange(1, R.RADIUS + 1)
    for i in range(n):
        for s in range(per):
            e = i * per + s
            k, j = e % R.N_BINS, e // R.N_BINS
            y, x = R.REACH + ((j + s) & 7), SLOT_X[s] + j
            ys[i, s], xs[i, s] = y, x
            m10, m01 = R.sweep_moments(k)
            img[i, y + R.DISC_DY, x + R.DISC_DX] = 0
            if m10:
                img[i, y, x + int(np.sign(m10)) * d] = R._axis_values(abs(m10))[1:]
            if m01:
                img[i, y + int(np.sign(m01)) * d, x] = R._axis_values(abs(m01))[1:]
    keys = R.make_keys(rng, ys, xs, W)
    return img, blur, keys, np.full(n, per, np.int32), H, W


def test_distinct_window_bytes_in_every_bin_narrow_and_wide(gpu):
    case = _case("lds_every_bin", _every_bin)
    keys, ref = case[2], case[6]
    # any two bytes of a 37 x 52 window at most two rows apart differ
    for dr in range(0, 3):
        for dc in range(-51, 52):
            assert (dr, dc) == (0, 0) or (PAT_A * dr + PAT_B * dc) % PAT_M != 0
    y, x = _yx(keys, W)
    assert fast(y, x, H, W, R.REACH, True).all() and fast(y, x, H, W, R.RADIUS, False).all()
    a = (x - R.REACH) & 15
    e = np.arange(keys.size).reshape(keys.shape)
    assert (ref["angle"] == e % R.N_BINS).all()
    for form in (a <= 11, a > 11):
        assert set(ref["angle"][form].tolist()) == set(range(R.N_BINS))                # every bin, narrow and wide
    assert {(int(k), int(v)) for k, v in zip(ref["angle"].reshape(-1), a.reshape(-1))} == {(k, v) for k in range(R.N_BINS) for v in range(16)}
    pts = R.ROT.reshape(-1, 2)
    assert {int(pts[:, 0].min()), int(pts[:, 0].max()), int(pts[:, 1].min()), int(pts[:, 1].max())} == {-R.REACH, R.REACH}
    check(case)


# ---- case 4: the clamped path
def _near_the_edges():
    rng = np.random.default_rng(104)
    img = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    blur = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    edge_rows, edge_cols = (0, 5, 17, H - 18, H - 6, H - 1), (0, 7, 17, W - 18, W - 8, W - 1)
    pos = [(y, x) for y in edge_rows for x in range(W)] + [(y, x) for y in range(R.REACH, H - R.REACH) for x in edge_cols]
    ys, xs = np.array(pos).T
    keys = R.make_keys(rng, ys, xs, W)[None]
    return img, blur, keys, np.array([keys.shape[1]], np.int32), H, W


def test_keypoints_within_18_pixels_of_each_image_edge(gpu):
    case = _case("lds_edges", _near_the_edges)
    keys = case[2]
    y, x = _yx(keys[0], W)
    near = (y < R.REACH) | (y >= H - R.REACH) | (x < R.REACH) | (x >= W - R.REACH)
    assert near.all() and not fast(y, x, H, W, R.REACH, True).any()
    for edge in (y < R.REACH, y >= H - R.REACH, x < R.REACH, x >= W - R.REACH):
        assert edge.sum() >= 100
    assert (~fast(y, x, H, W, R.RADIUS, False)).sum() > 100 and fast(y, x, H, W, R.RADIUS, False).sum() > 100   # mixed pairs too
    check(case)
