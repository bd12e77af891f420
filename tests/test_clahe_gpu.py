"""vus_clahe_luts / vus_clahe_apply on the GPU against their numpy statement (tests/clahe_ref.py), bit for bit: tiles
with reflect padding on either axis and tiles that lie wholly in the padding, odd widths, pitched and unaligned rows, one
tile and the tile-count limit, image counts 1, 3 and 33, the image kinds that put every lane on one histogram bin, and
clip values from none to "never reached"; then Clahe.enhance, murky frames through run_sequence against the oracle chain
on the numpy-enhanced frames, and the rectifier and the enhancer together."""
import ctypes

import numpy as np
import pytest
import torch

import clahe_ref as C
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

# H, W, pitch_s, pitch_d, tiles_x, tiles_y
SHAPES = [(37, 51, 51, 51, 3, 2),          # reflect padding in y, odd widths and pitches
          (96, 128, 128, 128, 8, 8),       # whole tiles
          (77, 131, 144, 136, 4, 4),       # padding in both axes, padded rows
          (77, 131, 131, 131, 4, 4),       # the same, rows at odd addresses
          (64, 64, 64, 64, 1, 1),          # one tile
          (45, 80, 80, 80, 8, 8),          # T = 60: clip = 1 at limit 4.0
          (50, 50, 52, 52, 16, 16),        # tiles that lie wholly in the padding
          (90, 160, 160, 160, 32, 2)]      # the tile-count limit
COUNTS = (1, 3, 33)
FILL, SRC_FILL, LUT_FILL = 0xA5, 0x3C, 0x5A


def _kinds(H, W):
    k = C.image_kinds(3, H, W, seed=H * W)
    k["murky"] = C.murk(synth.stereo_frames(0, 2, H, W).reshape(4, H, W)[:3])        # a murky synthetic frame
    return k


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d_p%d_%d_t%dx%d" % s)
def case(request):
    H, W, ps, pd, tx, ty = request.param
    tw, th = C.tile_size(H, W, tx, ty)
    T = tw * th
    kinds = _kinds(H, W)
    # 33 images: every kind three times and 9 more random ones
    many = np.concatenate(list(kinds.values()) + [np.random.default_rng(1).integers(0, 256, (9, H, W), dtype=np.uint8)])
    assert len(many) == 33
    clips = (0, 1, C.clip_count(4.0, T), T + 5)
    ref = {clip: C.luts(many, tx, ty, clip) for clip in clips}                       # computed once, shared, never changed
    out = {clip: C.apply(many, ref[clip], tx, ty) for clip in clips}
    return dict(H=H, W=W, ps=ps, pd=pd, tx=tx, ty=ty, T=T, clips=clips, many=many, luts=ref, out=out,
                kind_at={name: 3 * i for i, name in enumerate(kinds)})


def _src(src_np, ps, skew=0):
    n, H, W = src_np.shape
    sbuf = torch.full((n * H * ps + 8,), SRC_FILL, dtype=torch.uint8, device="cuda")
    s = sbuf[skew:skew + n * H * ps].view(n, H, ps)
    s[:, :, :W] = torch.from_numpy(src_np).cuda()
    return sbuf, s


def _outside(buf, skew, size, view=None, W=None):
    """The bytes of `buf` around [skew, skew + size) and, with a pitched view, between W and the pitch."""
    parts = [buf[:skew].cpu().numpy(), buf[skew + size:].cpu().numpy()]
    if view is not None:
        parts.append(view[:, :, W:].cpu().numpy().reshape(-1))
    return np.concatenate(parts)


def gpu_luts(src_np, ps, tx, ty, clip, src_skew=0, lut_skew=0):
    from visual_underwater_slam_amd import _lib
    n, H, W = src_np.shape
    sbuf, s = _src(src_np, ps, src_skew)
    size = n * ty * tx * 256
    lbuf = torch.full((size + 8,), LUT_FILL, dtype=torch.uint8, device="cuda")
    _lib.call("vus_clahe_luts", s.data_ptr(), n, H, W, ps, tx, ty, int(clip), lbuf.data_ptr() + lut_skew, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert (_outside(lbuf, lut_skew, size) == LUT_FILL).all()
    assert (_outside(sbuf, src_skew, n * H * ps, s, W) == SRC_FILL).all() and np.array_equal(s[:, :, :W].cpu().numpy(), src_np)
    return lbuf[lut_skew:lut_skew + size].view(n, ty, tx, 256).cpu().numpy()


def gpu_apply(src_np, luts_np, ps, pd, tx, ty, src_skew=0, dst_skew=0, lut_skew=0, in_place=False):
    from visual_underwater_slam_amd import _lib
    n, H, W = src_np.shape
    sbuf, s = _src(src_np, ps, src_skew)
    lbuf = torch.full((luts_np.size + 8,), LUT_FILL, dtype=torch.uint8, device="cuda")
    lbuf[lut_skew:lut_skew + luts_np.size] = torch.from_numpy(np.ascontiguousarray(luts_np).reshape(-1)).cuda()
    if in_place:
        dbuf, d, pd, dst_skew, fill = sbuf, s, ps, src_skew, SRC_FILL
    else:
        dbuf = torch.full((n * H * pd + 8,), FILL, dtype=torch.uint8, device="cuda")
        d, fill = dbuf[dst_skew:dst_skew + n * H * pd].view(n, H, pd), FILL
    _lib.call("vus_clahe_apply", s.data_ptr(), n, H, W, ps, lbuf.data_ptr() + lut_skew, tx, ty, d.data_ptr(), pd,
              _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert (_outside(dbuf, dst_skew, n * H * pd, d, W) == fill).all()                 # pitch padding and the bytes around
    if not in_place:
        assert np.array_equal(s[:, :, :W].cpu().numpy(), src_np)
    return d[:, :, :W].cpu().numpy()


def _batches(case):
    """(first image, count) of every batch: each kind at 1 and 3 images, and the 33 together."""
    for name, at in case["kind_at"].items():
        for n in COUNTS[:2]:
            yield name, at, n
    yield "all", 0, COUNTS[2]


def test_luts_equal_reference(gpu, case):
    for clip in case["clips"]:
        for name, at, n in _batches(case):
            got = gpu_luts(case["many"][at:at + n], case["ps"], case["tx"], case["ty"], clip)
            assert np.array_equal(got, case["luts"][clip][at:at + n]), (name, n, clip)


def test_apply_equals_reference_on_random_tables(gpu, case):
    """The apply kernel on its own: any 256 bytes are a table."""
    rng = np.random.default_rng(case["H"])
    tx, ty = case["tx"], case["ty"]
    for n in COUNTS:
        src = case["many"][:n]
        tables = rng.integers(0, 256, (n, ty, tx, 256), dtype=np.uint8)
        got = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty)
        assert np.array_equal(got, C.apply(src, tables, tx, ty)), n


def test_pair_equals_reference(gpu, case):
    tx, ty = case["tx"], case["ty"]
    for clip in case["clips"]:
        for name, at, n in _batches(case):
            src = case["many"][at:at + n]
            got = gpu_apply(src, gpu_luts(src, case["ps"], tx, ty, clip), case["ps"], case["pd"], tx, ty)
            assert np.array_equal(got, case["out"][clip][at:at + n]), (name, n, clip)
    # the statement itself: tiles = 1 x 1 without a clip is global equalisation
    if (tx, ty) == (1, 1):
        img, T = case["many"][0], case["T"]
        want = ((np.cumsum(np.bincount(img.reshape(-1), minlength=256)) * 255 + T // 2) // T).astype(np.uint8)[img]
        assert np.array_equal(case["out"][0][0], want)


def test_buffers_off_a_dword_boundary(gpu, case):
    """Buffers that start 1 .. 3 bytes off a 4-byte boundary: bytewise loads, stores and table writes, the same bytes."""
    tx, ty, clip = case["tx"], case["ty"], case["clips"][2]
    src = case["many"][:3]
    for ss, ds, ls in ((1, 0, 0), (0, 3, 0), (0, 0, 1), (2, 1, 3), (3, 2, 2)):
        tables = gpu_luts(src, case["ps"], tx, ty, clip, src_skew=ss, lut_skew=ls)
        assert np.array_equal(tables, case["luts"][clip][:3]), (ss, ls)
        got = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty, src_skew=ss, dst_skew=ds, lut_skew=ls)
        assert np.array_equal(got, case["out"][clip][:3]), (ss, ds, ls)


def test_in_place_equals_out_of_place_and_runs_repeat(gpu, case):
    tx, ty, clip = case["tx"], case["ty"], case["clips"][2]
    for n in COUNTS:
        src, tables = case["many"][:n], case["luts"][clip][:n]
        a = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty)
        b = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty)
        c = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty, in_place=True)
        d = gpu_apply(src, tables, case["ps"], case["pd"], tx, ty, src_skew=1, in_place=True)
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(a, case["out"][clip][:n])
        assert np.array_equal(gpu_luts(src, case["ps"], tx, ty, clip), gpu_luts(src, case["ps"], tx, ty, clip))


def test_more_images_than_a_grid_axis_holds(gpu):
    """65538 images of 6 x 10: a workgroup takes a second image.  The images repeat with period 5, so does the reference."""
    from visual_underwater_slam_amd import _lib
    n, h, w, tx, ty, clip = 65538, 6, 10, 2, 2, 2
    base = np.random.default_rng(9).integers(0, 256, (5, h, w), dtype=np.uint8)
    src = np.tile(base, (-(-n // 5), 1, 1))[:n]
    want_l, want = C.luts(base, tx, ty, clip), C.clahe(base, tx, ty, clip)
    d = torch.from_numpy(src).cuda()
    tables = torch.full((n, ty, tx, 256), LUT_FILL, dtype=torch.uint8, device="cuda")
    out = torch.full_like(d, FILL)
    st = _lib.current_stream_ptr()
    _lib.call("vus_clahe_luts", d.data_ptr(), n, h, w, w, tx, ty, clip, tables.data_ptr(), st)
    _lib.call("vus_clahe_apply", d.data_ptr(), n, h, w, w, tables.data_ptr(), tx, ty, out.data_ptr(), w, st)
    torch.cuda.synchronize()
    assert np.array_equal(tables.cpu().numpy(), np.tile(want_l, (-(-n // 5), 1, 1, 1))[:n])
    assert np.array_equal(out.cpu().numpy(), np.tile(want, (-(-n // 5), 1, 1))[:n])


def test_invalid_arguments_are_rejected_with_a_message(gpu):
    from visual_underwater_slam_amd import _lib
    lib = _lib.load()
    img = torch.zeros((1, 64, 96), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(img)
    tables = torch.zeros((1, 8, 8, 256), dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ok_l = [P(img), 1, 64, 96, 96, 8, 8, 3, P(tables), None]
    ok_a = [P(img), 1, 64, 96, 96, P(tables), 8, 8, P(out), 96, None]
    assert lib.vus_clahe_luts(*ok_l) == 0 and lib.vus_clahe_apply(*ok_a) == 0

    def bad(fn, ok, changes, word):
        a = list(ok)
        for i, v in changes.items():
            a[i] = v
        assert fn(*a) == -1 and word in lib.vus_last_error(), (changes, lib.vus_last_error())

    L, A = lib.vus_clahe_luts, lib.vus_clahe_apply
    for i in (0, 8):
        bad(L, ok_l, {i: None}, b"null")
    for i in (0, 5, 8):
        bad(A, ok_a, {i: None}, b"null")
    for fn, ok, tx, ty in ((L, ok_l, 5, 6), (A, ok_a, 6, 7)):
        bad(fn, ok, {1: 0}, b"n_img=0")
        bad(fn, ok, {2: 0}, b"H=0")
        bad(fn, ok, {3: 40000, 4: 40000}, b"W=40000")
        bad(fn, ok, {4: 95}, b"pitch_s=95")
        bad(fn, ok, {2: 32767, 3: 32767, 4: 70000, tx: 32, ty: 32}, b"2^31")
        bad(fn, ok, {tx: 33}, b"tiles_x=33")
        bad(fn, ok, {ty: 0}, b"tiles_y=0")
        bad(fn, ok, {2: 3, ty: 8}, b"tiles_y=8 pads H=3")
        bad(fn, ok, {3: 5, 4: 8, tx: 16}, b"tiles_x=16 pads W=5")
        bad(fn, ok, {2: 4096, 3: 4096, 4: 4096, tx: 1, ty: 1}, b"T=16777216")
    bad(L, ok_l, {7: -1}, b"clip=-1")
    bad(A, ok_a, {9: 95}, b"pitch_d=95")
    torch.cuda.synchronize()


# -- the host object and the sequence -----------------------------------------------------------------------------------

KF, H, W = 6, 360, 640


def test_clahe_object_equals_reference(gpu):
    from visual_underwater_slam_amd import clahe
    F = 3
    raw = C.murk(synth.stereo_frames(0, F, H, W))
    raw[0, 1] = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    en = clahe.Clahe(H, W)
    assert en.clip == 56 and en.tile_size == (80, 45)
    want = C.clahe(raw.reshape(2 * F, H, W), 8, 8, en.clip).reshape(F, 2, H, W)
    d = torch.from_numpy(raw).cuda()
    out = en.enhance(d)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), raw)
    assert np.array_equal(en.luts.cpu().numpy(), C.luts(raw.reshape(2 * F, H, W), 8, 8, en.clip))
    tables = en.luts
    assert en.enhance(d) is out and en.luts is tables                       # both buffers are reused
    mine = torch.empty_like(d)
    assert en.enhance(d, out=mine) is mine and torch.equal(mine, out)
    flat = en.enhance(d.view(2 * F, H, W)[:4], out=torch.empty((4, H, W), dtype=torch.uint8, device="cuda"))
    assert np.array_equal(flat.cpu().numpy(), want.reshape(2 * F, H, W)[:4]) and en.luts is tables    # fewer images: no new buffer
    work = d.clone()
    assert en.enhance(work, out=work) is work and np.array_equal(work.cpu().numpy(), want)            # in place
    with pytest.raises(ValueError, match="expected"):
        en.enhance(d[:, :, :-1].contiguous())
    # clip_limit = 0: no clipping
    plain = clahe.Clahe(H, W, tiles=(4, 3), clip_limit=0)
    assert plain.clip == 0
    assert np.array_equal(plain.enhance(d).cpu().numpy(), C.clahe(raw.reshape(2 * F, H, W), 4, 3, 0).reshape(F, 2, H, W))


@pytest.fixture(scope="module")
def scene():
    return synth.scene_sequence(KF, H, W)


def test_murky_frames_through_run_sequence_match_the_oracle_chain(gpu, oracle, scene):
    """Trajectory error is not asserted: on this scene the noise-free IMU and DVL carry the trajectory even with the few
    dozen stereo factors the murky frames give, so it tells nothing."""
    from oracle import chain
    from visual_underwater_slam_amd import clahe, sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    murky = C.murk(scene["frames"])
    d = torch.from_numpy(murky).cuda()
    en = clahe.Clahe(H, W)
    results, seq, st = sequence.run_sequence(d, scene["poses_init"], scene["imu"], scene["dvl"], disparity_sign=1, enhancer=en)
    _, _, st_plain = sequence.run_sequence(d, scene["poses_init"], scene["imu"], scene["dvl"], disparity_sign=1)
    enhanced = C.clahe(murky.reshape(2 * KF, H, W), 8, 8, en.clip).reshape(KF, 2, H, W)
    fe = chain.frontend(enhanced, 2000, **sequence.SEQUENCE_PARAMS)
    cam = np.array([*synth.INTRINSIC, -synth.BASELINE_M, 1920, 1080, 0.0])          # disparity_sign = +1
    fac = chain.factors(fe, scene["poses_init"], cam, scene["K"], sequence.GATE_PX)
    assert np.array_equal(st["ids"].cpu().numpy(), fe["ids"])
    assert np.array_equal(st["factors"]["obs_meas"].cpu().numpy(), fac["obs_meas"])
    op, _, _, _, _, orep = chain.optimise(fac, scene, KF, scene["K"], scene["sigma"], scene["prior_sigmas"])
    got = np.stack([results.atPose3(X(i)).flat12() for i in range(KF)])
    assert seq.optimizer.report().status == 0 and orep["status"] == 0
    assert np.abs(got - op).max() < 1e-6 * max(1.0, np.abs(op).max())
    n_enh, n_plain = int((st["frontend"].stereo_idx >= 0).sum()), int((st_plain["frontend"].stereo_idx >= 0).sum())
    print(f"stereo matches: murky {n_plain}, enhanced {n_enh}; stereo factors {len(fac['obs_meas'])}")
    assert n_enh >= 10 * n_plain
    assert np.array_equal(d.cpu().numpy(), murky)                                    # the caller's frames are untouched


def test_rectifier_and_enhancer_together(gpu, scene):
    """Raw rig frames -> rectifier -> enhancer: the images that reach the detector, read from the objects' buffers."""
    import rectify_ref as R
    from visual_underwater_slam_amd import clahe, rectify, sequence
    from visual_underwater_slam_amd.frontend import default_camera
    rig = R.Rig("radtan", H, W)
    rectifier = rectify.StereoRectifier.from_kalibr(rig.kalibr(), (H, W), new_camera=default_camera(H, W))
    en = clahe.Clahe(H, W)
    raw = torch.from_numpy(C.murk(R.raw_frames(rig, scene["poses_gt"]))).cuda()
    _, _, st = sequence.run_sequence(raw, scene["poses_init"], scene["imu"], scene["dvl"], disparity_sign=1, rectifier=rectifier,
                                     enhancer=en)
    rect = R.remap(raw.cpu().numpy().reshape(2 * KF, H, W), rectifier.maps_host)
    assert np.array_equal(rectifier.rectify(raw).cpu().numpy().reshape(2 * KF, H, W), rect)
    want = C.clahe(rect, 8, 8, en.clip)
    assert np.array_equal(en.enhanced.cpu().numpy().reshape(2 * KF, H, W), want)
    assert np.array_equal(en.luts.cpu().numpy(), C.luts(rect, 8, 8, en.clip))
    assert int((st["frontend"].stereo_idx >= 0).sum()) > 0
