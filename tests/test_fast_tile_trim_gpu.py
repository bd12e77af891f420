"""The FAST tile body at the sizes where its phases change shape, against the plain numpy reference of tests/fast_ref.py,
bit for bit: one tile, 2 x 2 full tiles (block-tiled path), partial edge tiles (still block-tiled), odd edges (row-major
only) and 3 x 3 tiles (the one shape with a tile whose whole ring lies inside the image).

The images are chosen by what the strip pre-test lists per tile (a numpy replica of it is part of this file and its
counts are asserted BEFORE the GPU is called): no strip at all (every wave skips the per-pixel pre-test), 1-64, 65-128,
129-192, 193-256 and more than 256 strips (one to four waves at work, then a second trip), and all 884 (noise at
threshold 1: four trips, the work list full).  Dots and arc stamps sit on the tile edges x = 127 / 128 and y = 23 / 24 and
on the four-tile junction, with equal and unequal scores, so that non-max suppression reads the ring of the neighbouring
tile in both directions and a tie suppresses both pixels; more stamps sit 3 pixels from each image edge.

Every entry point that instantiates the tile body is run on every shape it accepts: vus_fast_score, vus_fast_detect with
and without smoothing, vus_fast_detect_adaptive on one list and on eight sub-lists, vus_fast_detect_adaptive_tiled
(planes and candidates), vus_fast_threshold_estimate (histogram and thresholds) and the three-call protocol with a retry
that the test forces and predicts."""
import functools

import numpy as np
import pytest

import fast_ref as R
from test_fast_adversarial_gpu import (_dev, _i32, _u32, assert_candidates, gpu_adaptive, gpu_adaptive_tiled, gpu_detect,
                                       gpu_estimate, gpu_protocol, gpu_score, region_counts)

pytestmark = pytest.mark.gpu

SHAPES = ((24, 128), (48, 256), (56, 272), (53, 261), (72, 384))
TILED_SHAPES = tuple(s for s in SHAPES if s[0] % 8 == 0 and s[1] % 16 == 0)
THR = 20                      # the threshold of everything but the noise image
SC_ROWS, SC_DW = R.TILE_H + 2, R.TILE_W // 4 + 2      # a tile's strips: its 24 x 32 and a ring of one
CLASSES = ((0, 0), (1, 64), (65, 128), (129, 192), (193, 256), (257, SC_ROWS * SC_DW))


# ---- the strip pre-test, restated: strip (gy, gx = 4 d) may hold a corner only if, with the (min, max) of the staged
# dwords N / S (three rows up / down), W / E (left / right) and its own first and last byte b0 / b3,
#   min(max(N, S), max(W, E, b0, b3)) > min(strip) + thr   or   max(min(N, S), min(W, E, b0, b3)) < max(strip) - thr;
# strips reaching into the 3-pixel frame of the image in y, or lying left of x = 0 or right of x = W - 4, are never listed.
def strip_pass_map(img, thr):
    """bool [H, D]: strip d (pixels 4 d .. 4 d + 3) of row y is listed by the tiles that hold it."""
    H, W = img.shape
    D = -(-W // 4)
    P = np.pad(img, ((3, 3), (4, 4 + 4 * D - W)), mode="edge").astype(np.int32)     # what staging replicates
    dw = P.reshape(H + 6, D + 2, 4)
    mn, mx = dw.min(axis=2), dw.max(axis=2)
    own_mn, own_mx = mn[3:-3, 1:-1], mx[3:-3, 1:-1]
    b0, b3 = dw[3:-3, 1:-1, 0], dw[3:-3, 1:-1, 3]
    n_mx, s_mx, n_mn, s_mn = mx[:-6, 1:-1], mx[6:, 1:-1], mn[:-6, 1:-1], mn[6:, 1:-1]
    w_mx, e_mx, w_mn, e_mn = mx[3:-3, :-2], mx[3:-3, 2:], mn[3:-3, :-2], mn[3:-3, 2:]
    hi = np.minimum(np.maximum(n_mx, s_mx), np.maximum(np.maximum(w_mx, e_mx), np.maximum(b0, b3)))
    lo = np.maximum(np.minimum(n_mn, s_mn), np.minimum(np.minimum(w_mn, e_mn), np.minimum(b0, b3)))
    ok = (hi > own_mn + thr) | (lo < own_mx - thr)
    ys, ds = np.arange(H)[:, None], np.arange(D)[None, :]
    return ok & (ys >= 3) & (ys < H - 3) & (4 * ds < W - 3)


def listed_strips_per_tile(img, thr):
    """int [tiles_y, tiles_x]: strips listed by each tile's pre-test (its own 24 x 32 strips plus the ring)."""
    H, W = img.shape
    ok = strip_pass_map(img, thr)
    ty, tx = -(-H // R.TILE_H), -(-W // R.TILE_W)
    out = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            y0, d0 = R.TILE_H * j - 1, (R.TILE_W // 4) * i - 1
            out[j, i] = ok[max(y0, 0):y0 + SC_ROWS, max(d0, 0):d0 + SC_DW].sum()
    return out


def class_of(count):
    return next(k for k, (lo, hi) in enumerate(CLASSES) if lo <= count <= hi)


# ---- images
def lay_arc(img, y, x, L, k, v):
    """The arc stamp of fast_ref.arc_stamp_image at a centre of the caller's choosing."""
    for j in range(L):
        q = (k + j) & 15
        img[y + R.CIRCLE_DY[q], x + R.CIRCLE_DX[q]] = v


def sparse_stamp_image(H, W, per_tile, seed):
    """Flat 100 with per_tile[t] arcs of 9 .. 16 (contrast THR + 3 .. THR + 40, either sign) on the 8-pixel grid of
    tile t, tiles in raster order (cycled)."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 100, np.uint8)
    t = 0
    for y0 in range(0, H, R.TILE_H):
        for x0 in range(0, W, R.TILE_W):
            cells = [(y, x) for y in range(y0 + 4, min(y0 + R.TILE_H, H - 3), 8) for x in range(x0 + 4, min(x0 + R.TILE_W, W - 3), 8)]
            want = per_tile[t % len(per_tile)]
            t += 1
            for c in rng.permutation(len(cells))[:want]:
                d = int(rng.integers(THR + 3, THR + 41)) * (1 if rng.random() < 0.5 else -1)
                lay_arc(img, *cells[c], int(rng.integers(9, 17)), int(rng.integers(0, 16)), 100 + d)
    return img


SPARSE_DENSITIES = ((0, 2, 7, 12), (17, 48, 4, 0), (10, 14, 48, 1))


def edge_xy(H, W):
    """The last column / row before the first tile edge (127, 23), or an inner one where the image has no such edge."""
    return (R.TILE_W - 1 if W > R.TILE_W + 12 else W // 2), (R.TILE_H - 1 if H > R.TILE_H + 12 else H // 2)


def dot_pairs(H, W):
    """Adjacent pixel pairs (first, second): across the vertical edge, across the horizontal edge, diagonally across it,
    and the upper row of the 2 x 2 block on the four-tile junction (its lower row is weaker than both)."""
    xe, ye = edge_xy(H, W)
    return (((6, xe), (6, xe + 1)), ((ye, 16), (ye + 1, 16)), ((ye, 32), (ye + 1, 33)),
            ((ye, xe), (ye, xe + 1)))


def junction_images(H, W):
    """Dark dots on a bright ground: an isolated pixel scores its full contrast - 1 and nothing around it scores, so of
    two adjacent dots the darker survives and equal ones tie (both suppressed).  Image 0: every pair equal; image 1: the
    first pixel of every pair of dot_pairs the stronger; image 2: the second.  Where the image has tile edges, arc
    stamps are centred on x = 127, x = 128, y = 23 and y = 24 as well; full rings sit 3 pixels from the image edges."""
    xe, ye = edge_xy(H, W)
    out = []
    for k in range(3):
        img = np.full((H, W), 180, np.uint8)
        for p, q in dot_pairs(H, W):
            img[p], img[q] = ((100, 100), (90, 100), (100, 90))[k]
        img[ye + 1, xe], img[ye + 1, xe + 1] = 120, 120
        if H > R.TILE_H + 12 and W > R.TILE_W + 12:
            lay_arc(img, 14, xe, 11, 5, 240)
            lay_arc(img, 34, xe + 1, 12, 13, 120 + k)
            lay_arc(img, ye, 56, 10, 2, 110 + k)
            lay_arc(img, ye + 1, 100, 16, 0, 250)
        for (y, x) in ((3, 3), (3, W - 4), (H - 4, 3), (H - 4, W - 4), (3, xe + 40), (H - 4, xe + 40)):
            lay_arc(img, y, x, 16, 0, 120 + 7 * k)
        out.append(img)
    return out


@functools.lru_cache(maxsize=None)
def images(shape):
    """(imgs [n, H, W], thr per image): blank, noise (threshold 1), the junction / edge images, the sparse family."""
    H, W = shape
    rng = np.random.default_rng(H * W)
    imgs = [np.full((H, W), 77, np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)]
    imgs += junction_images(H, W)
    imgs += [sparse_stamp_image(H, W, d, seed=k) for k, d in enumerate(SPARSE_DENSITIES)]
    thrs = [THR, 1] + [THR] * (len(imgs) - 2)
    return np.stack(imgs), thrs


@functools.lru_cache(maxsize=None)
def reference(shape, thr, border):
    """Reference candidates of every image of the shape at one threshold (None: at its own)."""
    imgs, thrs = images(shape)
    if thr is None:
        return [R.fast_detect(imgs[i], thrs[i], border)[0][0] for i in range(len(imgs))]
    return R.fast_detect(imgs, thr, border)[0]


@functools.lru_cache(maxsize=None)
def smoothing(shape):
    return R.blur7(images(shape)[0])


# ---- conditions on the images themselves (no GPU)
def check_conditions(shape):
    H, W = shape
    imgs, thrs = images(shape)
    counts = [listed_strips_per_tile(imgs[i], thrs[i]) for i in range(len(imgs))]
    assert counts[0].max() == 0, "the blank image lists a strip"
    if shape == (72, 384):
        assert counts[1][1, 1] == SC_ROWS * SC_DW, ("noise at threshold 1 lists every strip of the inner tile", counts[1])
    assert counts[1][0, 0] > 256, counts[1]
    for k in (0, 1, 2):                       # the dots: equal scores tie, unequal scores keep the stronger alone
        sc = R.fast_score(imgs[2 + k], THR)[0]
        keep = R.nms_survivors(sc[None], 3)[0]
        for p, q in dot_pairs(H, W):
            assert sc[p] >= THR and sc[q] >= THR, (shape, k, p, q)
            assert (sc[p] == sc[q], sc[p] > sc[q], sc[p] < sc[q])[k], (shape, k, p, q)
            assert keep[p] == (k == 1) and keep[q] == (k == 2), (shape, k, p, q)
        xe, ye = edge_xy(H, W)
        assert sc[ye + 1, xe] >= THR and not keep[ye + 1, xe] and not keep[ye + 1, xe + 1], (shape, k)
        for (y, x) in ((3, 3), (3, W - 4), (H - 4, 3), (H - 4, W - 4)):
            assert sc[y, x] >= THR and keep[y, x], (shape, k, y, x)
    return counts


def test_images_meet_their_conditions():
    """The per-tile listed-strip counts hit every class (over the shapes' sparse families; the multi-tile shapes hit
    them all on their own), the ties tie and the edge stamps score -- asserted here without a GPU as well as by every
    GPU test below before its first call."""
    seen = set()
    for shape in SHAPES:
        counts = check_conditions(shape)
        here = {class_of(c) for cs in counts[5:] for c in cs.ravel()} | {class_of(0)}
        if shape[0] > R.TILE_H and shape[1] > R.TILE_W:
            assert here == set(range(len(CLASSES))), (shape, [cs.tolist() for cs in counts[5:]])
        seen |= here
    assert seen == set(range(len(CLASSES)))


@pytest.fixture(scope="module")
def ready(gpu):
    for shape in SHAPES:
        check_conditions(shape)
    return True


def _pitch(W, k):
    return R.pitch_at(W, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_score(ready, shape):
    imgs, _ = images(shape)
    W = shape[1]
    for k, thr in enumerate((1, THR)):
        want = R.fast_score(imgs, thr)
        for pitch in (W, _pitch(W, k + 1)):
            assert np.array_equal(gpu_score(R.padded(imgs, pitch), W, thr), want), (shape, thr, pitch)


@pytest.mark.parametrize("shape", SHAPES)
def test_detect_at_a_fixed_threshold(ready, shape):
    imgs, _ = images(shape)
    H, W = shape
    for k, (thr, border) in enumerate(((1, 3), (THR, 3), (THR, 0), (THR, 5))):
        want = reference(shape, thr, border)
        buf = R.padded(imgs, _pitch(W, k))
        for want_blur in (True, False):
            keys, cnt, blur = gpu_detect(buf, W, thr, border, H * W, want_blur)
            assert_candidates(keys, cnt, want, H * W, (shape, thr, border, want_blur))
            if want_blur:
                assert np.array_equal(blur, smoothing(shape)), (shape, thr)


@pytest.mark.parametrize("shape", SHAPES)
def test_adaptive_on_one_list_and_on_eight(ready, shape):
    imgs, thrs = images(shape)
    H, W = shape
    n = len(imgs)
    want = reference(shape, None, 3)
    cap = 8 * 4096                              # a sub-list of 4095 slots holds any tile
    for k in range(2):
        pitch = _pitch(W, 2 * k)
        d = _dev(R.padded(imgs, pitch))
        for want_blur, c in ((True, cap), (False, cap), (True, 511)):       # eight sub-lists; one list; one list + smoothing
            keys, cnt, blur = gpu_adaptive(d, n, H, W, pitch, _i32(thrs), 3, c, want_blur)
            assert_candidates(_u32(keys), cnt.cpu().numpy(), want, c, (shape, pitch, want_blur, c))
            if want_blur:
                assert np.array_equal(blur.cpu().numpy(), smoothing(shape)), (shape, pitch, c)


@pytest.mark.parametrize("shape", TILED_SHAPES)
def test_adaptive_tiled_planes_and_candidates(ready, shape):
    from visual_underwater_slam_amd.frontend import untile_planes
    imgs, thrs = images(shape)
    H, W = shape
    n = len(imgs)
    want = reference(shape, None, 4)
    for k in range(2):
        pitch = _pitch(W, 3 * k)
        d = _dev(R.padded(imgs, pitch))
        cap = 8 * 4096
        keys, cnt, blur_t, img_t = gpu_adaptive_tiled(d, n, H, W, pitch, _i32(thrs), 4, cap)
        keys, cnt = _u32(keys), cnt.cpu().numpy()
        for i, w in enumerate(want):
            assert region_counts(w, H, W).max() <= cap // 8 - 1
            assert cnt[i] == len(w) and np.array_equal(np.sort(keys[i, :cnt[i]]), w), (shape, pitch, i)
        assert np.array_equal(untile_planes(blur_t, H, W).cpu().numpy(), smoothing(shape)), (shape, pitch)
        assert np.array_equal(untile_planes(img_t, H, W).cpu().numpy(), imgs), (shape, pitch)


@pytest.mark.parametrize("shape", SHAPES)
def test_threshold_estimate(ready, shape):
    imgs, _ = images(shape)
    H, W = shape
    n = len(imgs)
    for k, (thr, border, max_kp, stride) in enumerate(((THR, 3, 20, 1), (1, 0, 200, 2), (60, 4, 3, 3))):
        rh, rt = R.threshold_estimate(imgs, thr, border, max_kp, stride)
        pitch = _pitch(W, k)
        hist, thr_img = gpu_estimate(_dev(R.padded(imgs, pitch)), n, H, W, pitch, thr, border, max_kp, stride)
        assert np.array_equal(hist.cpu().numpy(), rh) and np.array_equal(thr_img.cpu().numpy(), rt), (shape, thr, stride)


def protocol_images(shape):
    """Two images that must be detected again, two that must not.  [0]: strong corners in the sampled tile only, weak
    ones elsewhere -- the estimate lands above the weak scores and the adaptive pass finds fewer than max_kp.  [1]:
    noise -- on eight sub-lists of cand_cap / 8 - 1 = 63 slots a tile overflows its sub-list.  [2], [3]: a sparse
    image and the blank one."""
    H, W = shape
    tx, ty = -(-W // R.TILE_W), -(-H // R.TILE_H)
    stride = tx * ty
    sampled = stride // 2
    rng = np.random.default_rng(5)
    a = np.full((H, W), 100, np.uint8)
    for t in range(stride):
        y0, x0 = (t // tx) * R.TILE_H, (t % tx) * R.TILE_W
        cells = [(y, x) for y in range(y0 + 4, min(y0 + R.TILE_H, H - 3), 8) for x in range(x0 + 4, min(x0 + R.TILE_W, W - 3), 8)]
        for (y, x) in cells[::2]:
            lay_arc(a, y, x, 12, int(rng.integers(0, 16)), 100 + (120 + int(rng.integers(0, 20)) if t == sampled else 45))
    imgs = np.stack([a, rng.integers(0, 256, (H, W), dtype=np.uint8), sparse_stamp_image(H, W, (5, 9), seed=9),
                     np.full((H, W), 9, np.uint8)])
    return imgs, stride


def predicted_retries(imgs, shape, thr, border, max_kp, stride, cap, path):
    """(thr_img, images vus_fast_detect_retry must list) by the header's rule: an image whose adaptive pass ran above thr
    and found fewer than max_kp, or whose list -- or, on eight sub-lists, one sub-list of cap / 8 - 1 slots -- overflowed."""
    H, W = shape
    _, rt = R.threshold_estimate(imgs, thr, border, max_kp, stride)
    at_rt = [R.fast_detect(imgs[i], int(rt[i]), border)[0][0] for i in range(len(imgs))]
    return rt, [i for i in range(len(imgs))
                if (rt[i] > thr and len(at_rt[i]) < max_kp) or len(at_rt[i]) > cap
                or (path != "single" and region_counts(at_rt[i], H, W).max() > cap // 8 - 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_three_call_protocol_with_a_forced_retry(ready, shape):
    """max_kp 40 (8 on one tile): the estimate from the strong tile alone overshoots image 0.  max_kp 2000: no threshold
    above the floor qualifies, the noise image is detected at thr and overflows a sub-list of 63 slots (eight sub-lists)
    or the whole list of 128 (one list: a true overflow, reported with its true count after the retry)."""
    H, W = shape
    imgs, stride = protocol_images(shape)
    thr, border = 10, 3
    want, wcnt = R.fast_detect(imgs, thr, border)
    paths = ("regions", "single") + (("tiled",) if shape in TILED_SHAPES else ())
    for max_kp in (40 if stride > 1 else 8, 2000):
        rkp, rkc = R.select_topk(want, max_kp)
        for path in paths:
            cap = 128 if path == "single" and max_kp == 2000 else 512
            rt, predicted = predicted_retries(imgs, shape, thr, border, max_kp, stride, cap, path)
            if max_kp == 2000:
                assert 1 in predicted and 2 not in predicted and 3 not in predicted, (shape, path, predicted)
            elif stride > 1:
                assert 0 in predicted and 2 not in predicted and 3 not in predicted, (shape, path, predicted)
            pitch = _pitch(W, 1)
            kp, kc, cnt, thr_img, retried = gpu_protocol(R.padded(imgs, pitch), W, thr, border, max_kp, stride, cap, path)
            what = (shape, max_kp, path, cnt.tolist(), wcnt.tolist(), thr_img.tolist(), retried)
            assert np.array_equal(thr_img, rt), what
            assert retried == predicted, what
            for i in range(len(imgs)):
                if wcnt[i] <= cap or cnt[i] <= cap:
                    assert kc[i] == rkc[i] and np.array_equal(kp[i], rkp[i]), (i,) + what
                else:
                    assert cnt[i] == wcnt[i], (i,) + what
