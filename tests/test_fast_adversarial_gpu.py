"""Every FAST entry point of the HIP library against the plain numpy reference of tests/fast_ref.py, bit for bit, on
adversarial images: contrasts exactly at the threshold, arcs of 7..16 at every start, saturated content, plateaus and
ties, thresholds up to 254, borders 0..4 and past the middle, odd widths, pitch > W with junk in the padding, and
candidates concentrated in one tile column (the layout that overflows one of the eight candidate sub-lists of the
adaptive detector long before the list is full).  Candidates compare as sets together with the true count."""
import numpy as np
import pytest
import torch

import fast_ref as R

pytestmark = pytest.mark.gpu

THRS = (1, 2, 9, 10, 40, 41, 127, 128, 200, 253, 254)
BORDERS = (0, 1, 2, 3, 4, 31, 10 ** 4)
SHAPES = ((7, 7), (8, 9), (23, 127), (24, 128), (25, 129), (49, 257), (97, 131), (96, 1024))
_KEEP = []   # device inputs stay referenced until the module is done (a freed tensor's memory could be reused while a
             # launched kernel still reads it)


def _L():
    import visual_underwater_slam_amd._lib as L
    return L


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return t


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _i32(a):
    return torch.tensor(np.asarray(a, np.int32), device="cuda")


def gpu_score(buf, W, thr):
    L = _L()
    n, H, pitch = buf.shape
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    L.call("vus_fast_score", _dev(buf).data_ptr(), n, H, W, pitch, int(thr), out.data_ptr(), L.current_stream_ptr())
    return out.cpu().numpy()


def gpu_blur(buf, W):
    L = _L()
    n, H, pitch = buf.shape
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    L.call("vus_blur7", _dev(buf).data_ptr(), n, H, W, pitch, out.data_ptr(), L.current_stream_ptr())
    return out.cpu().numpy()


def gpu_detect(buf, W, thr, border, cap, want_blur):
    L = _L()
    n, H, pitch = buf.shape
    keys = torch.full((n, cap), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    blur = torch.empty((n, H, W), dtype=torch.uint8, device="cuda") if want_blur else None
    L.call("vus_fast_detect", _dev(buf).data_ptr(), n, H, W, pitch, int(thr), int(border), L.ptr(blur), keys.data_ptr(), cap,
           cnt.data_ptr(), L.current_stream_ptr())
    return _u32(keys), cnt.cpu().numpy(), None if blur is None else blur.cpu().numpy()


def gpu_adaptive(d_img, n, H, W, pitch, thr_img_t, border, cap, want_blur, keys=None, cnt=None):
    """vus_fast_detect_adaptive on device buffers (keys / cnt reused by the protocol); returns (keys, cnt, blur) tensors."""
    L = _L()
    keys = torch.full((n, cap), 7, dtype=torch.int32, device="cuda") if keys is None else keys
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda") if cnt is None else cnt
    blur = torch.empty((n, H, W), dtype=torch.uint8, device="cuda") if want_blur else None
    L.call("vus_fast_detect_adaptive", d_img.data_ptr(), n, H, W, pitch, thr_img_t.data_ptr(), int(border), L.ptr(blur),
           keys.data_ptr(), cap, cnt.data_ptr(), L.current_stream_ptr())
    return keys, cnt, blur


def gpu_adaptive_tiled(d_img, n, H, W, pitch, thr_img_t, border, cap, keys=None, cnt=None):
    L = _L()
    keys = torch.full((n, cap), 7, dtype=torch.int32, device="cuda") if keys is None else keys
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda") if cnt is None else cnt
    blur_t = torch.empty((n, H * W), dtype=torch.uint8, device="cuda")
    img_t = torch.empty((n, H * W), dtype=torch.uint8, device="cuda")
    L.call("vus_fast_detect_adaptive_tiled", d_img.data_ptr(), n, H, W, pitch, thr_img_t.data_ptr(), int(border),
           blur_t.data_ptr(), img_t.data_ptr(), keys.data_ptr(), cap, cnt.data_ptr(), L.current_stream_ptr())
    return keys, cnt, blur_t, img_t


def gpu_estimate(d_img, n, H, W, pitch, thr, border, max_kp, stride):
    L = _L()
    hist = torch.full((n, 256), 5, dtype=torch.int32, device="cuda")
    thr_img = torch.zeros(n, dtype=torch.int32, device="cuda")
    L.call("vus_fast_threshold_estimate", d_img.data_ptr(), n, H, W, pitch, int(thr), int(border), int(max_kp), int(stride),
           hist.data_ptr(), thr_img.data_ptr(), L.current_stream_ptr())
    return hist, thr_img


def gpu_protocol(buf, W, thr, border, max_kp, stride, cap, path):
    """estimate -> adaptive (path: "regions" = with blur, cap >= 512; "single" = without blur; "tiled") -> retry ->
    vus_select_topk.  Returns (kp [n, max_kp], kp_count, cand_count, thr_img, retried images)."""
    L = _L()
    n, H, pitch = buf.shape
    d = _dev(buf)
    st = L.current_stream_ptr()
    _, thr_img = gpu_estimate(d, n, H, W, pitch, thr, border, max_kp, stride)
    keys = torch.full((n, cap), 7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    if path == "tiled":
        gpu_adaptive_tiled(d, n, H, W, pitch, thr_img, border, cap, keys, cnt)
    else:
        gpu_adaptive(d, n, H, W, pitch, thr_img, border, cap, path == "regions", keys, cnt)
    lst = torch.zeros(n, dtype=torch.int32, device="cuda")
    m = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("vus_fast_detect_retry", d.data_ptr(), n, H, W, pitch, int(thr), thr_img.data_ptr(), int(max_kp), int(border),
           keys.data_ptr(), cap, cnt.data_ptr(), lst.data_ptr(), m.data_ptr(), st)
    kp = torch.empty((n, max_kp), dtype=torch.int32, device="cuda")
    kc = torch.empty(n, dtype=torch.int32, device="cuda")
    L.call("vus_select_topk", keys.data_ptr(), cnt.data_ptr(), n, cap, int(max_kp), kp.data_ptr(), kc.data_ptr(), st)
    return (_u32(kp), kc.cpu().numpy(), cnt.cpu().numpy(), thr_img.cpu().numpy(),
            sorted(lst.cpu().numpy()[:int(m.item())].tolist()))


def region_counts(keys, H, W):
    """Candidates per sub-list of the REGIONS path (tile t of the 128 x 24 raster into sub-list t mod 8)."""
    tx = -(-W // R.TILE_W)
    pos = np.asarray(keys, np.uint32) & np.uint32(0xFFFFFF)
    tile = (pos // W) // R.TILE_H * tx + (pos % W) // R.TILE_W
    return np.bincount(tile % 8, minlength=8)


def assert_candidates(keys, cnt, want, cap, what):
    """keys [n, cap] / cnt [n] of a single-list detection against the reference sets: the true count always; the exact
    set when it fits, otherwise cap distinct true candidates."""
    for i, w in enumerate(want):
        assert cnt[i] == len(w), (what, i, int(cnt[i]), len(w))
        got = keys[i, :min(cnt[i], cap)]
        if len(w) <= cap:
            assert np.array_equal(np.sort(got), w), (what, i)
        else:
            assert len(np.unique(got)) == cap and np.isin(got, w).all(), (what, i)


def _family(k, H, W, thr):
    """The k-th adversarial family at this shape (cycled by the grid tests)."""
    f = k % 5
    if f == 0:
        return R.saturated_images(H, W, thr, seed=k)
    if f == 1:
        return R.plateau_images(H, W)[k % 20::3]
    if f == 2:
        return np.stack([R.tie_image(H, W, min(thr, 240), step=5 + k % 4),
                         R.plateau_images(H, W, 100, min(255, 100 + thr + 1))[k % 20]])
    if f == 3:
        return R.corner_free_images(H, W, thr)
    s = R.saturated_images(H, W, thr, seed=k)
    return np.stack([s[0], s[4], s[7], R.concentrated_image(H, W, col=(k % 3))])


def test_fast_score_at_every_threshold_and_pitch(gpu):
    """vus_fast_score == the definition on the arc stamps (contrast thr - 1 .. thr + 2 around 0 / 1 / thr / 127 / 128 /
    255 - thr / 254 / 255) and on saturated images, at every thr and every pitch; the padding is 0 / 255 junk."""
    for t, thr in enumerate(THRS):
        stamps, _ = R.arc_stamp_images(thr)
        sat = R.saturated_images(97, 131, thr, seed=t)
        want_s, want_n = R.fast_score(stamps, thr), R.fast_score(sat, thr)
        for pitch in R.pitches(stamps.shape[2]):
            assert np.array_equal(gpu_score(R.padded(stamps, pitch), stamps.shape[2], thr), want_s), (thr, pitch)
        for pitch in R.pitches(131):
            assert np.array_equal(gpu_score(R.padded(sat, pitch), 131, thr), want_n), (thr, pitch)


@pytest.mark.parametrize("shape", SHAPES)
def test_smoothing_on_saturated_noise_and_stamps(gpu, shape):
    """vus_blur7, and the blur_out of vus_fast_detect and of vus_fast_detect_adaptive on both list paths (eight
    sub-lists with cand_cap >= 512, one list below), == the reference smoothing on 0 / 255-heavy content at every
    pitch."""
    H, W = shape
    sat = R.saturated_images(H, W, 41, seed=H)
    stamps, _ = R.arc_stamp_images(10)
    imgs = np.concatenate([sat, np.ascontiguousarray(stamps[[0, 7], :H, :W]) if H <= 192 and W <= 259 else sat[:0]])
    n = len(imgs)
    want = R.blur7(imgs)
    thr_img = _i32([(1, 10, 128, 254)[i % 4] for i in range(n)])
    for k, pitch in enumerate(R.pitches(W)):
        buf = R.padded(imgs, pitch)
        assert np.array_equal(gpu_blur(buf, W), want), ("vus_blur7", pitch)
        _, _, b = gpu_detect(buf, W, (10, 254)[k % 2], (0, 31)[k % 2], 64, True)
        assert np.array_equal(b, want), ("vus_fast_detect", pitch)
        d = _dev(buf)
        for cap in (512, 511):
            _, _, b = gpu_adaptive(d, n, H, W, pitch, thr_img, 3, cap, True)
            assert np.array_equal(b.cpu().numpy(), want), ("vus_fast_detect_adaptive", cap, pitch)


@pytest.mark.parametrize("shape", SHAPES + ((720, 1280),))
def test_detect_over_threshold_border_pitch_grid(gpu, shape):
    """vus_fast_detect, with and without blur_out, over a sample of the thr x border x pitch grid on the adversarial
    families: candidate set and true count bit for bit; a cand_cap below the count keeps the true count and cap true
    candidates."""
    H, W = shape
    j = SHAPES.index(shape) if shape in SHAPES else len(SHAPES)
    ks = range(len(THRS)) if H * W <= 100_000 else range(j % 3, len(THRS), 4)
    for k in ks:
        thr = THRS[k]
        imgs = _family(k + j, H, W, thr)
        imgs = imgs[:3] if H * W > 200_000 else imgs
        border = BORDERS[(k + j) % len(BORDERS)]
        pitch = R.pitch_at(W, k + j)
        want, wcnt = R.fast_detect(imgs, thr, border)
        buf = R.padded(imgs, pitch)
        keys, cnt, blur = gpu_detect(buf, W, thr, border, H * W, (k % 2) == 0)
        assert_candidates(keys, cnt, want, H * W, (shape, thr, border, pitch))
        if blur is not None:
            assert np.array_equal(blur, R.blur7(imgs)), (shape, pitch)
        if wcnt.max() > 3:
            cap = int(wcnt.max()) // 2
            keys, cnt, _ = gpu_detect(buf, W, thr, border, cap, (k % 2) == 1)
            assert_candidates(keys, cnt, want, cap, (shape, thr, border, pitch, cap))


@pytest.mark.parametrize("shape", ((25, 129), (97, 131), (96, 1024), (192, 259)))
def test_adaptive_with_mixed_per_image_thresholds(gpu, shape):
    """vus_fast_detect_adaptive with thr_img mixing 1, 10, 128 and 254 == the reference at each image's threshold, on
    the single-list path (no blur_out, or cand_cap < 512) and on the eight-sub-list path, where a sub-list that
    outgrows cand_cap / 8 - 1 must be reported as cand_count > cand_cap with only true candidates kept."""
    H, W = shape
    sat = R.saturated_images(H, W, 10, seed=W)
    imgs = np.stack([sat[0], sat[1], sat[3], sat[6], sat[7], R.tie_image(H, W, 9), R.concentrated_image(H, W, col=1)])
    if shape == (192, 259):
        imgs = np.concatenate([imgs, R.arc_stamp_images(128)[0][[0, 4, 7]]])
    n = len(imgs)
    thrs = [(1, 10, 128, 254)[i % 4] for i in range(n)]
    want = [R.fast_detect(imgs[i], thrs[i], 3)[0][0] for i in range(n)]
    for k, pitch in enumerate(R.pitches(W)[:2]):
        d = _dev(R.padded(imgs, pitch))
        for cap, blur in ((H * W, False), (511, True), (H * W, True), (4096, True), (512, True)):
            keys, cnt, _ = gpu_adaptive(d, n, H, W, pitch, _i32(thrs), 3, cap, blur)
            keys, cnt = _u32(keys), cnt.cpu().numpy()
            if not (blur and cap >= 512):
                assert_candidates(keys, cnt, want, cap, (shape, cap, pitch))
                continue
            for i, w in enumerate(want):
                if region_counts(w, H, W).max() <= cap // 8 - 1:
                    assert cnt[i] == len(w) and np.array_equal(np.sort(keys[i, :cnt[i]]), w), (shape, cap, i)
                else:
                    assert cnt[i] > cap, (shape, cap, i)
                    kept = keys[i][keys[i] != R.KEY_INVALID]
                    assert len(np.unique(kept)) == len(kept) and np.isin(kept, w).all(), (shape, cap, i)


@pytest.mark.parametrize("shape,pitch_k", (((24, 128), 0), ((96, 1024), 1), ((200, 272), 3), ((720, 1280), 2)))
def test_adaptive_tiled_planes_and_candidates(gpu, shape, pitch_k):
    """vus_fast_detect_adaptive_tiled on whole-block shapes: candidate set as the reference at each image's threshold,
    the un-tiled blur plane == the reference smoothing and the un-tiled raw plane == the image."""
    from visual_underwater_slam_amd.frontend import untile_planes
    H, W = shape
    sat = R.saturated_images(H, W, 41, seed=3)
    imgs = np.stack([sat[0], sat[4], sat[6], R.tie_image(H, W, 41), R.concentrated_image(H, W, col=0)])
    n = len(imgs)
    thrs = [(254, 1, 128, 41, 10)[i] for i in range(n)]
    want = [R.fast_detect(imgs[i], thrs[i], 4)[0][0] for i in range(n)]
    pitch = R.pitch_at(W, pitch_k)
    d = _dev(R.padded(imgs, pitch))
    cap = H * W if H * W >= 512 else 4096
    keys, cnt, blur_t, img_t = gpu_adaptive_tiled(d, n, H, W, pitch, _i32(thrs), 4, cap)
    keys, cnt = _u32(keys), cnt.cpu().numpy()
    for i, w in enumerate(want):
        assert region_counts(w, H, W).max() <= cap // 8 - 1
        assert cnt[i] == len(w) and np.array_equal(np.sort(keys[i, :cnt[i]]), w), (shape, i)
    assert np.array_equal(untile_planes(blur_t, H, W).cpu().numpy(), R.blur7(imgs))
    assert np.array_equal(untile_planes(img_t, H, W).cpu().numpy(), imgs)


@pytest.mark.parametrize("case", [((96, 1024), 10, 31, 2000, 32), ((720, 1280), 10, 31, 2000, 32),
                                  ((97, 131), 41, 3, 5, 1), ((49, 257), 128, 0, 3, 2), ((192, 259), 200, 4, 40, 3),
                                  ((96, 1024), 254, 31, 1, 4), ((96, 1024), 60, 2, 30, 1)])
def test_threshold_estimate_hist_and_thresholds(gpu, case):
    """vus_fast_threshold_estimate: hist and thr_img == the header's rule, including thr > 40 (the sample detected at
    f = thr), every-tile and first-tile-only samples, at two pitches."""
    (H, W), thr, border, max_kp, stride = case
    sat = R.saturated_images(H, W, thr, seed=7)
    imgs = np.stack([sat[0], sat[6], sat[7], R.tie_image(H, W, min(thr, 240)), R.concentrated_image(H, W, col=0)])
    n = len(imgs)
    rh, rt = R.threshold_estimate(imgs, thr, border, max_kp, stride)
    for pitch in (W, R.pitches(W)[-1]):
        hist, thr_img = gpu_estimate(_dev(R.padded(imgs, pitch)), n, H, W, pitch, thr, border, max_kp, stride)
        assert np.array_equal(hist.cpu().numpy(), rh) and np.array_equal(thr_img.cpu().numpy(), rt), pitch


def _protocol_images(H, W, thr):
    sat = R.saturated_images(H, W, thr, seed=11)
    return np.stack([R.tie_image(H, W, min(thr, 240)), R.tie_image(H, W, min(thr, 240), step=6), sat[0], sat[2], sat[7],
                     R.concentrated_image(H, W, col=3 if W > 3 * R.TILE_W else 0)])


@pytest.mark.parametrize("case", [((97, 131), 10, 3, 4096, 1), ((96, 1024), 10, 3, 4096, 32), ((96, 1024), 41, 3, 4096, 1),
                                  ((96, 512), 10, 3, 4096, 32), ((96, 256), 10, 3, 2048, 32), ((192, 259), 128, 31, 1024, 2),
                                  ((96, 1024), 10, 3, 2048, 32)])
def test_three_call_protocol_equals_detection_at_thr(gpu, case):
    """estimate -> adaptive -> retry, then vus_select_topk == the reference top-K at thr, keys and counts bit for bit,
    for K in {1, inside the tie, count - 1, count, count + 1} on every list path -- including images whose candidates
    crowd into one sub-list (a 96 x 1024 image with noise in one tile column: 1229 candidates, all in the sub-list of
    511 slots that cand_cap 4096 gives).  An image that truly overflows cand_cap keeps its true count."""
    (H, W), thr, border, cap, stride = case
    imgs = _protocol_images(H, W, thr)
    want, wcnt = R.fast_detect(imgs, thr, border)
    fits = wcnt <= cap
    c_tie, c_conc = int(wcnt[0]), int(wcnt[-1])
    Ks = sorted({1, max(1, c_tie // 2), max(1, c_tie - 1), c_tie + 1, max(1, c_conc - 1), c_conc, c_conc + 1})
    paths = ("regions", "single") + (("tiled",) if H % 8 == 0 and W % 16 == 0 else ())
    for K in Ks:
        K = min(K, 8192)
        rkp, rkc = R.select_topk(want, K)
        for path in paths:
            for pitch in (W, R.pitch_at(W, 2)) if path != "single" else (W,):
                kp, kc, cnt, thr_img, retried = gpu_protocol(R.padded(imgs, pitch), W, thr, border, K, stride, cap, path)
                what = (K, path, pitch, cnt.tolist(), wcnt.tolist(), thr_img.tolist(), retried)
                for i in range(len(imgs)):
                    if fits[i] or cnt[i] <= cap:    # a list that fits at thr_img (>= K candidates) holds the top K
                        assert kc[i] == rkc[i] and np.array_equal(kp[i], rkp[i]), (i,) + what
                    else:                           # a true overflow at thr: reported with its true count
                        assert cnt[i] == wcnt[i], (i,) + what


def _frontend_run(frames, H, W, K, **kw):
    from visual_underwater_slam_amd.frontend import StereoOrbFrontend, ImageProcessorParams
    fe = StereoOrbFrontend(H, W, max_frames=frames.shape[0], params=ImageProcessorParams(max_features=K, **kw))
    res = fe.process(frames)          # raises if it reports an overflow of cand_cap
    torch.cuda.synchronize()
    return fe, {k: getattr(res, k).cpu().numpy().copy() for k in ("kp_keys", "kp_count", "desc", "angle", "stereo_idx",
                                                                  "stereo_dist")}


@pytest.mark.parametrize("H,W,levels", [(720, 1024, 1), (720, 512, 1), (720, 1024, 3)])
def test_frontend_with_texture_in_one_tile_column(gpu, H, W, levels):
    """StereoOrbFrontend (adaptive; the tiled single-level path, or a 3-level pyramid whose levels use the eight
    sub-lists) on a stereo pair whose texture lies in one 128-pixel tile column of a flat frame -- an underwater frame
    with one textured object against open water -- raises no overflow and equals adaptive_fast=False bit for bit.
    At 720 x 1024 all ~8800 candidates fall into one sub-list of 5759 slots (cand_cap 46080 fits them eight times); at
    720 x 512 the tile column of x = 256 .. 383 fills two sub-lists of 4095 slots with ~4400 each."""
    left = R.concentrated_image(H, W, col=3 if W > 4 * R.TILE_W else 2, seed=1)
    right = np.roll(left, -6, axis=1)
    frames = torch.from_numpy(np.stack([left, right])[None]).cuda()
    K = 2000 if levels == 1 else 1500
    fe_a, a = _frontend_run(frames, H, W, K, n_levels=levels)
    assert fe_a.tiled == (levels == 1)
    _, b = _frontend_run(frames, H, W, K, n_levels=levels, adaptive_fast=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (a["kp_count"] == K).all() if levels == 1 else (a["kp_count"] > K // 2).all()
