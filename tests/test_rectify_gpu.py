"""vus_rectify_plan / vus_rectify_remap on the GPU against their numpy statement (tests/rectify_ref.py), bit for bit, on
every path of the kernel: staged and direct tiles, partial tiles, pitched and unaligned rows, image counts around the
frame group; StereoRectifier.rectify; and raw frames through run_sequence against the ideal render of the same scene.

Which tiles are staged depends on the LDS budget (VUS_RECTIFY_LDS_BYTES = 8192): an image that fits it as a whole (37 x 51)
is staged whatever its map holds, so "no tile staged" is asserted for the random map only on shapes over the budget, and
the x5 shrink, whose footprint is 320 x 80 pixels, gets a shape wide enough for it (100 x 340)."""
import ctypes

import numpy as np
import pytest
import torch

import rectify_ref as R
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

# H, W, pitch_s, pitch_d
SHAPES = [(37, 51, 51, 51),          # smaller than one tile; W and the pitches no multiple of 4
          (96, 128, 128, 128),       # whole tiles
          (77, 131, 144, 136),       # partial tiles, padded rows
          (77, 131, 131, 131),       # the same, rows at odd addresses: bytewise staging and stores
          (100, 340, 340, 340)]      # W a multiple of 4 but not of 64; wide enough for the shrink to leave the budget
COUNTS = (1, 3, 9, 33)               # images per map; 8 boxes are staged per pass and the frame group is 32: 9 = one
                                     # pass and one image more, 33 = one full group and one image more
FILL = 0xA5


def maps_of(H, W):
    lens = R.Rig("radtan", H, W).maps()[0]
    half = lens.copy()
    half[:, W // 2:] = R.random_map(H, W, 11)[:, W // 2:]
    return {"identity": R.identity_map(H, W), "shift+33": R.shift_map(H, W, 33, 33), "shift-33": R.shift_map(H, W, -33, -33),
            "radtan": lens, "equidistant": R.Rig("equidistant", H, W).maps()[1], "rot180": R.rotate180_map(H, W),
            "shrink5": R.shrink_map(H, W), "random": R.random_map(H, W, 7), "half": half}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d_p%d_%d" % s)
def case(request):
    H, W, ps, pd = request.param
    maps = maps_of(H, W)
    src = np.random.default_rng(H * W).integers(0, 256, (2 * max(COUNTS), H, W), dtype=np.uint8)
    return dict(H=H, W=W, ps=ps, pd=pd, maps=maps, src=src, plan=R.plan(np.stack(list(maps.values()))))


def gpu_plan(maps_np):
    from visual_underwater_slam_amd import _lib
    n, H, W = maps_np.shape
    maps = torch.from_numpy(np.ascontiguousarray(maps_np)).cuda()
    boxes = torch.full((n, -(-H // R.TILE_H), -(-W // R.TILE_W), 4), -7, dtype=torch.int32, device="cuda")
    _lib.call("vus_rectify_plan", _lib.ptr(maps), n, H, W, _lib.ptr(boxes), _lib.current_stream_ptr())
    return maps, boxes


def gpu_remap(src_np, maps, boxes, ps, pd, src_skew=0, dst_skew=0):
    """src_np [n, H, W] -> (out [n, H, W], the bytes of dst beyond W).  *_skew: the buffer starts that many bytes off a
    4-byte boundary."""
    from visual_underwater_slam_amd import _lib
    n, H, W = src_np.shape
    sbuf = torch.full((n * H * ps + 8,), 0x3C, dtype=torch.uint8, device="cuda")
    dbuf = torch.full((n * H * pd + 8,), FILL, dtype=torch.uint8, device="cuda")
    s = sbuf[src_skew:src_skew + n * H * ps].view(n, H, ps)
    d = dbuf[dst_skew:dst_skew + n * H * pd].view(n, H, pd)
    s[:, :, :W] = torch.from_numpy(src_np).cuda()
    _lib.call("vus_rectify_remap", s.data_ptr(), n, H, W, ps, _lib.ptr(maps), _lib.ptr(boxes), maps.shape[0], d.data_ptr(), pd,
              _lib.current_stream_ptr())
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    guard = np.concatenate([dbuf[:dst_skew].cpu().numpy(), dbuf[dst_skew + n * H * pd:].cpu().numpy(), out[:, :, W:].reshape(-1)])
    return out[:, :, :W], guard


def test_plan_equals_reference(gpu, case):
    names = list(case["maps"])
    _, boxes = gpu_plan(np.stack(list(case["maps"].values())))
    got = boxes.cpu().numpy()
    assert np.array_equal(got, case["plan"])
    w = {k: got[i, ..., 2] for i, k in enumerate(names)}
    # both kernel paths are taken
    for k in ("identity", "shift+33", "shift-33", "radtan", "equidistant"):
        assert (w[k] > 0).all(), k
    H, W = case["H"], case["W"]
    if ((W + 6) & ~3) * H > R.LDS_BYTES:                    # else the whole image fits the budget
        assert (w["random"] == 0).all()
        assert (w["half"][:, 0] > 0).all() and (w["half"][:, -1] == 0).all()
    if W >= 320:
        assert (w["shrink5"] == 0).any()


@pytest.mark.parametrize("n_maps", (1, 2))
def test_remap_equals_reference(gpu, case, n_maps):
    names = list(case["maps"])
    ps, pd = case["ps"], case["pd"]
    staged = direct = 0
    for i, k in enumerate(names):
        sel = [k] if n_maps == 1 else [k, names[(i + 4) % len(names)]]       # the second map is of another kind
        mnp = np.stack([case["maps"][s] for s in sel])
        maps, boxes = gpu_plan(mnp)
        bw = boxes.cpu().numpy()[..., 2]
        staged, direct = staged + int((bw > 0).sum()), direct + int((bw == 0).sum())
        for n in COUNTS:
            for n_img in ((n,) if n_maps == 1 else (n, 2 * n)):              # odd counts too: the maps get unequal shares
                src = case["src"][:n_img]
                out, guard = gpu_remap(src, maps, boxes, ps, pd)
                assert np.array_equal(out, R.remap(src, mnp)), (sel, n_img)
                assert (guard == FILL).all(), (sel, n_img)
    assert staged > 0 and (direct > 0 or ((case["W"] + 6) & ~3) * case["H"] <= R.LDS_BYTES)


def test_remap_is_repeatable_and_the_boxes_are_only_a_schedule(gpu, case):
    """Two runs give the same bytes; all-zero boxes (every tile gathers from global memory), the boxes of ANOTHER map
    and arbitrary numbers in `boxes` change nothing: a box that does not cover its tile is not used."""
    ps, pd, H, W = case["ps"], case["pd"], case["H"], case["W"]
    src = case["src"][:9]
    rng = np.random.default_rng(3)
    for k in ("radtan", "rot180", "half"):
        mnp = case["maps"][k][None]
        want = R.remap(src, mnp)
        maps, boxes = gpu_plan(mnp)
        a, _ = gpu_remap(src, maps, boxes, ps, pd)
        b, _ = gpu_remap(src, maps, boxes, ps, pd)
        assert np.array_equal(a, b) and np.array_equal(a, want)
        _, other = gpu_plan(case["maps"]["identity"][None])
        whole = torch.tensor([0, 0, W, H], dtype=torch.int32, device="cuda").expand_as(boxes).contiguous()
        junk = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, tuple(boxes.shape), dtype=np.int64).astype(np.int32)).cuda()
        small = torch.from_numpy(rng.integers(-4, 80, tuple(boxes.shape), dtype=np.int64).astype(np.int32)).cuda()
        for bx in (torch.zeros_like(boxes), other, whole, junk, small):
            out, guard = gpu_remap(src, maps, bx, ps, pd)
            assert np.array_equal(out, want), k
            assert (guard == FILL).all()


def test_rows_off_a_dword_boundary(gpu, case):
    """Buffers that start 1..3 bytes off a 4-byte boundary: bytewise staging (src) and bytewise stores (dst)."""
    src = case["src"][:3]
    mnp = np.stack([case["maps"]["equidistant"], case["maps"]["half"]])
    maps, boxes = gpu_plan(mnp)
    want = R.remap(src, mnp)
    for ss, ds in ((1, 0), (0, 3), (2, 1)):
        out, guard = gpu_remap(src, maps, boxes, case["ps"], case["pd"], src_skew=ss, dst_skew=ds)
        assert np.array_equal(out, want), (ss, ds)
        assert (guard == FILL).all(), (ss, ds)


def test_invalid_arguments_are_rejected_with_a_message(gpu):
    from visual_underwater_slam_amd import _lib
    lib = _lib.load()
    maps, boxes = gpu_plan(R.identity_map(32, 64)[None])
    img = torch.zeros((1, 32, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(img)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = [P(img), 1, 32, 64, 64, P(maps), P(boxes), 1, P(out), 64, None]
    assert lib.vus_rectify_remap(*ok) == 0

    def bad(i, v, word):
        a = list(ok)
        a[i] = v
        assert lib.vus_rectify_remap(*a) == -1 and word in lib.vus_last_error(), (i, lib.vus_last_error())

    for i in (0, 5, 6, 8):
        bad(i, None, b"null")
    bad(7, 0, b"n_maps")
    bad(1, 0, b"n_img")
    bad(4, 63, b"pitch")
    bad(9, 60, b"pitch")
    bad(2, 0, b"H=")
    bad(3, 40000, b"W=")
    assert lib.vus_rectify_plan(None, 1, 32, 64, P(boxes), None) == -1 and b"null" in lib.vus_last_error()
    assert lib.vus_rectify_plan(P(maps), 1, 32, 64, None, None) == -1 and b"null" in lib.vus_last_error()
    assert lib.vus_rectify_plan(P(maps), 0, 32, 64, P(boxes), None) == -1 and b"n_maps" in lib.vus_last_error()
    assert lib.vus_rectify_plan(P(maps), 1, 32, 0, P(boxes), None) == -1 and b"W=" in lib.vus_last_error()
    torch.cuda.synchronize()


# -- the host object and the sequence -----------------------------------------------------------------------------------

KF, H, W = 6, 360, 640


@pytest.fixture(scope="module")
def rig():
    return R.Rig("radtan", H, W)


@pytest.fixture(scope="module")
def rectifier(gpu, rig):
    from visual_underwater_slam_amd import rectify
    from visual_underwater_slam_amd.frontend import default_camera
    return rectify.StereoRectifier.from_kalibr(rig.kalibr(), (H, W), new_camera=default_camera(H, W))


def test_stereo_rectifier_equals_reference(gpu, rig, rectifier):
    F = 3
    raw = np.random.default_rng(5).integers(0, 256, (F, 2, H, W), dtype=np.uint8)
    want = R.remap(raw.reshape(2 * F, H, W), rectifier.maps_host).reshape(F, 2, H, W)
    d = torch.from_numpy(raw).cuda()
    out = rectifier.rectify(d)
    assert np.array_equal(out.cpu().numpy(), want)
    assert rectifier.rectify(d) is out                                  # the buffer is reused
    mine = torch.empty_like(d)
    assert rectifier.rectify(d, out=mine) is mine and torch.equal(mine, out)
    assert np.array_equal(rectifier.maps.cpu().numpy(), rectifier.maps_host)
    boxes = rectifier.boxes.cpu().numpy()
    assert np.array_equal(boxes, R.plan(rectifier.maps_host)) and (boxes[..., 2] > 0).all()
    assert (rectifier.maps_host != rig.maps()).mean() <= 1e-3
    cam = rectifier.cam_array(1).cpu().numpy()
    assert np.allclose(cam, [*rectifier.camera, -synth.BASELINE_M, W, H, 0.0], rtol=0, atol=1e-12)


def test_raw_frames_through_run_sequence_match_the_ideal_render(gpu, rig, rectifier):
    """The product has no CPU fallback, so the reference of this test is run_sequence on the ideal (already rectified)
    render of the same scene; the margins are the issue's: bilinear resampling moves FAST corners by a fraction of a pixel
    while the noise model is sigma = 10 px."""
    from visual_underwater_slam_amd import sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import L, X
    s = synth.scene_sequence(KF, H, W)
    raw = R.raw_frames(rig, s["poses_gt"], xp=torch, device=gpu)

    def run(frames, **kw):
        res, seq, st = sequence.run_sequence(frames, s["poses_init"], s["imu"], s["dvl"], disparity_sign=1, **kw)
        seen = np.nonzero(st["factors"]["lm_first"].cpu().numpy() >= 0)[0]
        pts = res.point3_block(L(0) + seen.astype(np.int64))
        got = np.stack([res.atPose3(X(i)).flat12() for i in range(KF)])
        return dict(status=seq.optimizer.report().status, stereo=int((st["frontend"].stereo_idx >= 0).sum()),
                    factors=int(st["factors"]["obs_frame"].numel()),
                    plane=float(np.median(np.abs(pts[:, 2] - synth.SCENE_PLANE_Z))),
                    err=float(np.linalg.norm(got[:, 9:] - s["poses_gt"][:, 9:], axis=1).max()))

    ideal = run(torch.from_numpy(s["frames"]).cuda())
    rect = run(raw, rectifier=rectifier)
    print("ideal", ideal, "\nrectified", rect)
    assert ideal["status"] == 0 and rect["status"] == 0
    assert rect["stereo"] >= 0.8 * ideal["stereo"]
    assert rect["factors"] >= 0.8 * ideal["factors"]
    assert rect["plane"] <= 1.25 * ideal["plane"]
    assert rect["err"] <= max(2.0 * ideal["err"], 0.005)


def test_run_sequence_refuses_a_rectifier_with_another_camera(gpu, rig):
    from visual_underwater_slam_amd import rectify, sequence
    s = synth.scene_sequence(2, H, W, render=False)
    auto = rectify.StereoRectifier.from_kalibr(rig.kalibr(), (H, W))           # fitted camera, not default_camera
    frames = torch.zeros((2, 2, H, W), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="new_camera=default_camera"):
        sequence.run_sequence(frames, s["poses_init"], s["imu"], s["dvl"], rectifier=auto)
