"""The CPU oracle's FAST detector against the plain numpy reference of tests/fast_ref.py (written from include/vus.h),
bit for bit, on adversarial content the synthetic frames never produce: contrasts exactly at the threshold, arcs of 8
and 9 at every start, saturated images, plateaus and ties, corner-free ramps, thresholds up to 254, borders 0..4 and
past the middle, odd widths and pitch > W with junk in the padding."""
import numpy as np
import pytest

import fast_ref as R

THRS = (1, 2, 9, 10, 40, 41, 127, 128, 200, 253, 254)
SMALL_SHAPES = ((7, 7), (8, 9), (23, 127), (24, 128), (25, 129), (49, 257), (97, 131))


def _p(a):
    from oracle.oracle import _p as p
    return p(a)


def oracle_score(O, buf, W, thr):
    n, H, pitch = buf.shape
    out = np.empty((n, H, W), np.uint8)
    assert O.lib().vus_fast_score_cpu(_p(buf), n, H, W, pitch, int(thr), _p(out)) == 0
    return out


def oracle_blur(O, buf, W):
    n, H, pitch = buf.shape
    out = np.empty((n, H, W), np.uint8)
    assert O.lib().vus_blur7_cpu(_p(buf), n, H, W, pitch, _p(out)) == 0
    return out


def oracle_detect(O, buf, W, thr, border, cap=None, blur=False):
    n, H, pitch = buf.shape
    cap = cap or H * W
    keys = np.full((n, cap), R.KEY_INVALID, np.uint32)
    cnt = np.zeros(n, np.int32)
    bl = np.empty((n, H, W), np.uint8) if blur else None
    assert O.lib().vus_fast_detect_cpu(_p(buf), n, H, W, pitch, int(thr), int(border), _p(bl), _p(keys), cap, _p(cnt)) == 0
    return keys, cnt, bl


def oracle_estimate(O, buf, W, thr, border, max_kp, stride):
    n, H, pitch = buf.shape
    hist = np.zeros((n, 256), np.int32)
    thr_img = np.zeros(n, np.int32)
    assert O.lib().vus_fast_threshold_estimate_cpu(_p(buf), n, H, W, pitch, int(thr), int(border), int(max_kp), int(stride),
                                                   _p(hist), _p(thr_img)) == 0
    return hist, thr_img


def check_against_oracle(O, imgs, thr, border, pitch):
    """fast_score, fast_detect (set and true count) and blur7 of the oracle at this pitch == the reference."""
    n, H, W = imgs.shape
    buf = R.padded(imgs, pitch)
    assert np.array_equal(oracle_score(O, buf, W, thr), R.fast_score(imgs, thr)), (thr, pitch)
    want, wcnt = R.fast_detect(imgs, thr, border)
    keys, cnt, blur = oracle_detect(O, buf, W, thr, border, blur=True)
    assert np.array_equal(cnt, wcnt), (thr, border, pitch)
    for i in range(n):
        assert np.array_equal(np.sort(keys[i, :cnt[i]]), want[i]), (i, thr, border, pitch)
    assert np.array_equal(blur, R.blur7(imgs)), pitch
    return want, wcnt


@pytest.mark.parametrize("thr", THRS)
def test_arc_stamps_score_exactly_at_the_threshold(oracle, thr):
    """Every arc stamp's centre scores what the definition says (an arc of 9 only from L >= 9, the clamped contrast
    minus one, strict comparisons: contrast thr is not a corner at thr, thr + 1 is), in the reference and the oracle;
    then the whole stamp images agree bit for bit, at a pitch and border that change with thr."""
    imgs, lays = R.arc_stamp_images(thr)
    sc = R.fast_score(imgs, thr)
    osc = oracle_score(oracle, np.ascontiguousarray(imgs), imgs.shape[2], thr)
    n_corner = 0
    for i, (c, laid) in enumerate(zip(R.stamp_centre_values(thr), lays)):
        for (y, x, L, k, sgn, dl) in laid:
            s = R.stamp_centre_score(c, L, sgn, dl)
            want = s if s >= thr else 0
            assert sc[i, y, x] == want and osc[i, y, x] == want, (c, y, x, L, k, sgn, dl, sc[i, y, x], osc[i, y, x])
            n_corner += want > 0
    assert n_corner > 0 or thr >= 253            # at 253 / 254 clamping leaves no contrast above thr for some c only
    i = THRS.index(thr)
    border = (0, 1, 2, 3, 4, 31, 100)[i % 7]
    pitch = R.pitch_at(imgs.shape[2], i)
    check_against_oracle(oracle, imgs, thr, border, pitch)


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_saturated_plateau_and_corner_free_images(oracle, shape):
    """Binary, salt-and-pepper, noise, checkerboards / stripes and ramps at every small shape, over thresholds up to
    254, borders 0..4 / 31 / past the middle and every pitch."""
    H, W = shape
    j = SMALL_SHAPES.index(shape)
    for t, thr in enumerate(THRS):
        fam = (R.saturated_images(H, W, thr, seed=t), R.plateau_images(H, W),
               R.plateau_images(H, W, 100, min(255, 100 + thr + 1)), R.corner_free_images(H, W, thr))[t % 4]
        border = (0, 1, 2, 3, 4, 31, max(H, W) // 2)[(t + j) % 7]
        pitch = R.pitch_at(W, t + j)
        _, cnt = check_against_oracle(oracle, fam, thr, border, pitch)
        if t % 4 == 3:
            assert (cnt == 0).all()                  # corner-free by construction


def test_corner_free_images_have_no_corners(oracle):
    imgs = R.corner_free_images(40, 67, 9)
    for thr in (1, 9, 10):
        assert not R.fast_score(imgs, thr).any() and not oracle_score(oracle, imgs, 67, thr).any()


def test_large_shapes_and_a_border_that_leaves_nothing(oracle):
    """(96, 1024) and (720, 1280) noise and stamps at two pitches; border >= H / 2 leaves no candidate."""
    for (H, W), thr, pitch in (((96, 1024), 10, 1024 + 13), ((720, 1280), 41, 1344)):
        imgs = np.stack([R.saturated_images(H, W, thr, seed=3)[6], R.tie_image(H, W, thr),
                         R.concentrated_image(H, W, col=3)])
        check_against_oracle(oracle, imgs, thr, 31, pitch)
        _, cnt = check_against_oracle(oracle, imgs[:1], thr, H // 2, W)
        assert cnt[0] == 0


@pytest.mark.parametrize("thr", (1, 10, 41, 128, 254))
def test_select_topk_cuts_inside_a_tie(oracle, thr):
    """Hundreds of equal scores: the top-K cut falls inside the tie and is decided by raster order; also K = 1,
    count - 1, count, count + 1, and a list the detector truncated (count > cap)."""
    H, W = 97, 131
    imgs = np.stack([R.tie_image(H, W, min(thr, 240)), R.saturated_images(H, W, thr)[0]])
    want, wcnt = R.fast_detect(imgs, thr, 3)
    keys, cnt, _ = oracle_detect(oracle, np.ascontiguousarray(imgs), W, thr, 3)
    assert np.array_equal(cnt, wcnt)
    c0 = int(wcnt[0])
    for K in sorted({1, max(1, c0 // 2), max(1, c0 - 1), max(1, c0), c0 + 1}):
        kp, kc = oracle.select_topk(keys, cnt, K)
        rkp, rkc = R.select_topk(want, K)
        assert np.array_equal(kp, rkp) and np.array_equal(kc, rkc), K
    if wcnt[1] > 4:                                   # a truncated list: kp_count = min(K, cap), keys from the kept ones
        cap = int(wcnt[1]) // 2
        keys, cnt, _ = oracle_detect(oracle, np.ascontiguousarray(imgs), W, thr, 3, cap=cap)
        assert cnt[1] == wcnt[1]
        kp, kc = oracle.select_topk(keys, cnt, cap + 5)
        rkp, rkc = R.select_topk([keys[i, :min(cnt[i], cap)] for i in range(2)], cap + 5)
        assert np.array_equal(kp, rkp) and np.array_equal(kc, rkc) and kc[1] == cap


@pytest.mark.parametrize("case", [((96, 1024), 10, 31, 2000, 32), ((720, 1280), 10, 31, 2000, 32),
                                  ((97, 131), 41, 3, 5, 1), ((49, 257), 128, 0, 3, 2), ((192, 259), 200, 4, 40, 3),
                                  ((96, 1024), 254, 31, 1, 4)])
def test_threshold_estimate_matches_the_reference(oracle, case):
    """hist and thr_img of the oracle's estimate == the header's rule, including thr > 40 (f = thr), strides that
    sample every tile or none past the first, and n_sampled clamped to 1."""
    (H, W), thr, border, max_kp, stride = case
    sat = R.saturated_images(H, W, thr, seed=7)
    imgs = np.stack([sat[0], sat[6], sat[7], R.tie_image(H, W, min(thr, 240)), R.concentrated_image(H, W, col=0)])
    for pitch in (W, R.pitches(W)[-1]):
        hist, thr_img = oracle_estimate(oracle, R.padded(imgs, pitch), W, thr, border, max_kp, stride)
        rh, rt = R.threshold_estimate(imgs, thr, border, max_kp, stride)
        assert np.array_equal(hist, rh) and np.array_equal(thr_img, rt), pitch
    assert (rt >= thr).all()


def test_oracle_retry_resolves_a_reported_overflow(oracle):
    """vus_fast_detect_retry_cpu lists an image whose count exceeds cand_cap (as the REGIONS path reports a sub-list
    overflow) and detects it again at thr: a list that fits comes back whole, a true overflow keeps its true count."""
    H, W, cap = 96, 1024, 4096
    imgs = np.stack([R.concentrated_image(H, W, col=3), R.saturated_images(H, W, 10)[6], R.tie_image(H, W, 10)])
    want, wcnt = R.fast_detect(imgs, 10, 3)
    assert wcnt[0] < cap < wcnt[1]
    keys = np.full((3, cap), R.KEY_INVALID, np.uint32)
    cnt = np.array([cap + 1, 0, cap + 7], np.int32)       # 0 and 2: reported overflows (stale keys in 2), 1: too few
    thr_img = np.array([10, 60, 10], np.int32)
    keys[2, :5] = 123
    lst, m = np.zeros(3, np.int32), np.zeros(1, np.int32)
    assert oracle.lib().vus_fast_detect_retry_cpu(_p(imgs), 3, H, W, W, 10, _p(thr_img), 2000, 3, _p(keys), cap, _p(cnt),
                                                  _p(lst), _p(m)) == 0
    assert sorted(lst[:int(m[0])].tolist()) == [0, 1, 2]
    assert np.array_equal(cnt, wcnt)
    assert np.array_equal(np.sort(keys[0, :cnt[0]]), want[0])
    assert set(keys[1].tolist()) <= set(want[1].tolist())
