"""vus_stereo_refine on the GPU against its numpy statement (tests/subpixel_ref.py): disp_q8 and status EQUAL, on small
images with keypoints on every border, tables with indices and counts out of range, every window / search size at the
limits, and list lengths that cross the 16-lane group, the wave and the workgroup.  Then its consumers: the u1 column of
feature_tracks and the depths of vus_stereo_pair_pose_q8 (against loop_ref / subpixel_ref, by the rule of
tests/test_loop_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import loop_ref as R
import subpixel_ref as S
import test_loop_gpu as TL

pytestmark = pytest.mark.gpu

H, W = 40, 72
DISP_SENTINEL, STATUS_SENTINEL = 0x7F7F7F7F, 0x5A
INT_MAX = 2 ** 31 - 1


# counts of three frames (left, right per frame): above max_kp (clamped), cutting live slots off, negative, zero
ODD_COUNTS = {"above_and_empty": lambda K: (K + 9, max(K - 2, 1), 2 ** 30, -3, 0, K),
              "cutting": lambda K: (K // 2, K, K, K // 2, -5, K)}


def images(kind, F, pitch, seed):
    """uint8 [2F, H, pitch]; the columns past W hold other noise (never read)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (2 * F, H, pitch), dtype=np.uint8)
    if kind == "ramp":
        img[:, :, :W] = (3 * np.arange(W)).astype(np.uint8)[None, None, :]
        img[1::2, :, :W] = (3 * np.arange(W) + 7).astype(np.uint8)[None, None, :]      # a shift of 7/3 columns
    elif kind == "constant":
        img[:, :, :W] = 131
    elif kind == "equal":
        img[1::2] = img[0::2]
    else:
        assert kind == "noise"
    return img


def tables(F, K, seed, counts="full"):
    """Keys at (0,0), (W-1,H-1), on every border and anywhere inside, right columns at both ends of the row (so that
    xr + s - half_win falls below 0 and beyond W-1), stereo indices in range and out of it (-1, nr, INT_MAX, negative)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, W, (2 * F, K))
    y = rng.integers(0, H, (2 * F, K))
    special = [(0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (1, 1),
               (W - 2, H - 2)]
    for n in range(2 * F):
        slots = rng.permutation(K)[:len(special)]
        for s, (sx, sy) in zip(slots, special):
            x[n, s], y[n, s] = sx, sy
    edge = rng.random((F, K)) < 0.3                                 # right keypoints hugging either end of the row
    x[1::2][edge] = rng.choice(np.array([0, 1, 2, W - 3, W - 2, W - 1]), int(edge.sum()))
    keys = ((rng.integers(0, 256, (2 * F, K)).astype(np.uint32) << 24) | (y * W + x).astype(np.uint32))
    cnt = np.full(2 * F, K, np.int32)
    if counts != "full":
        cnt = np.array(ODD_COUNTS[counts](K), np.int32)
        assert len(cnt) == 2 * F
    sidx = rng.integers(0, K, (F, K)).astype(np.int32)
    bad = rng.random((F, K))
    nr = np.array([S.T._clamp_count(cnt[2 * f + 1], K) for f in range(F)])[:, None] * np.ones((1, K), np.int64)
    for lo, hi, val in ((0.0, 0.1, -1), (0.1, 0.15, None), (0.15, 0.2, INT_MAX), (0.2, 0.25, -7), (0.25, 0.28, -2 ** 31)):
        pick = (bad >= lo) & (bad < hi)
        sidx[pick] = nr[pick].astype(np.int32) if val is None else val
    return sidx, keys, cnt


def run_gpu(img, sidx, keys, cnt, half_win, search, offset=1):
    """The images sit `offset` bytes into their allocation (an odd base address); outputs are prefilled with sentinels."""
    from visual_underwater_slam_amd import _lib as L
    F, K = sidx.shape
    pitch = img.shape[2]
    buf = torch.zeros(img.size + offset, dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    si, ke, co = d(sidx.astype(np.int32)), d(keys.view(np.int32)), d(cnt.astype(np.int32))
    disp = torch.full((F, K), DISP_SENTINEL, dtype=torch.int32, device="cuda")
    status = torch.full((F, K), STATUS_SENTINEL, dtype=torch.uint8, device="cuda")
    L.call("vus_stereo_refine", buf.data_ptr() + offset, F, img.shape[1], W, pitch, si.data_ptr(),
           ke.data_ptr(), co.data_ptr(), K, half_win, search, disp.data_ptr(), status.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(si.cpu().numpy(), sidx) and np.array_equal(co.cpu().numpy(), cnt)       # inputs left alone
    return disp.cpu().numpy(), status.cpu().numpy()


def check(kind, F, K, pitch, half_win, search, seed, counts="full", offset=1):
    img = images(kind, F, pitch, seed)
    sidx, keys, cnt = tables(F, K, seed + 1000, counts)
    want_d, want_s = S.refine(img, W, sidx, keys, cnt, half_win, search)
    got_d, got_s = run_gpu(img, sidx, keys, cnt, half_win, search, offset)
    assert not (got_d == DISP_SENTINEL).any() and not (got_s == STATUS_SENTINEL).any()            # every slot is written
    bad = np.argwhere((got_d != want_d) | (got_s != want_s))
    assert len(bad) == 0, (len(bad), [(f, i, got_d[f, i], want_d[f, i], got_s[f, i], want_s[f, i]) for f, i in bad[:5]])
    return want_d, want_s, got_d, got_s


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 64, 65, 257])
def test_list_lengths_across_the_group_the_wave_and_the_workgroup(gpu, K, F):
    want_d, want_s, _, _ = check("noise", F, K, (72, 80)[K % 2], 5, 5, seed=K + F)
    if K >= 64:
        assert (want_s == S.NONE).any() and (want_s != S.NONE).any()


@pytest.mark.parametrize("pitch", [72, 80])
@pytest.mark.parametrize("half_win,search", [(1, 1), (5, 5), (7, 8), (3, 8)])
@pytest.mark.parametrize("kind", ["noise", "ramp", "constant", "equal"])
def test_images_windows_and_pitches(gpu, kind, half_win, search, pitch):
    want_d, want_s, _, _ = check(kind, 3, 65, pitch, half_win, search, seed=7 * half_win + search)
    m = want_s != S.NONE
    assert m.sum() > 60
    if kind == "constant":
        assert (want_s[m] == S.EDGE).all()
    if kind == "ramp" and (half_win, search) != (1, 1):
        assert (want_s[m] == S.OK).any()


@pytest.mark.parametrize("half_win,search", [(1, 1), (5, 5), (7, 8), (3, 8)])
def test_every_column_on_either_side(gpu, half_win, search):
    """Every left column and every right column once per row parity: each position of a row relative to the image's edges,
    so both ways of loading a row (whole dwords inside the image row, clamped bytes at its ends) and the columns where
    one turns into the other."""
    rng = np.random.default_rng(11)
    img = images("noise", 1, 80, 12)
    i = np.arange(2 * W)
    xl, xr, y = i % W, (7 * i + 3) % W, rng.integers(0, H, 2 * W)
    assert set(xl) == set(xr) == set(range(W))
    keys = np.stack([(y * W + xl), (y * W + xr)]).astype(np.uint32) | np.uint32(5 << 24)
    sidx, cnt = i.astype(np.int32)[None, :], np.array([2 * W, 2 * W], np.int32)
    want_d, want_s = S.refine(img, W, sidx, keys, cnt, half_win, search)
    got_d, got_s = run_gpu(img, sidx, keys, cnt, half_win, search)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_s, want_s)
    assert (want_s != S.NONE).all()


@pytest.mark.parametrize("K", [17, 257])
@pytest.mark.parametrize("counts", list(ODD_COUNTS))
def test_counts_negative_and_above_max_kp(gpu, counts, K):
    want_d, want_s, _, _ = check("noise", 3, K, 80, 5, 5, seed=31, counts=counts)
    assert (want_s[0] != S.NONE).any()                   # frame 0 is live under either set of counts
    assert (want_s[2] == S.NONE).all()                   # frame 2: its left list is empty (0 or negative)
    if counts == "above_and_empty":
        assert (want_s[1] == S.NONE).all()               # frame 1: its right list is empty (negative)
    else:
        assert (want_s[0, K // 2:] == S.NONE).all() and (want_s[1] != S.NONE).any()


def test_aligned_base_address_and_two_runs_give_the_same_bits(gpu):
    a = check("noise", 3, 257, 80, 7, 8, seed=5, offset=0)
    b = check("noise", 3, 257, 80, 7, 8, seed=5, offset=1)
    c = check("noise", 3, 257, 80, 7, 8, seed=5, offset=1)
    for x, y in ((a, b), (b, c)):
        assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])


# ----------------------------------------------------------------------------------------------------------------------
# on a real front-end result, and the consumers

@pytest.fixture(scope="module")
def golden(gpu):
    from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_96x128.npz"))
    prm = ImageProcessorParams(max_features=64, border=20, cand_cap=2048, max_disparity=64, stereo_max_distance=80)
    fe = StereoOrbFrontend(96, 128, max_frames=1, params=prm)
    images_d = torch.from_numpy(g["img"][None]).cuda()
    res = fe.process(images_d)
    disp, status = fe.refine_stereo(res, images_d)
    torch.cuda.synchronize()
    host = dict(img=g["img"], sidx=res.stereo_idx.cpu().numpy(), keys=res.kp_keys.cpu().numpy().view(np.uint32),
                cnt=res.kp_count.cpu().numpy())
    return fe, res, images_d, disp, status, host


def test_front_end_result_equals_the_reference(golden):
    fe, res, images_d, disp, status, h = golden
    want_d, want_s = S.refine(h["img"], 128, h["sidx"], h["keys"], h["cnt"], 5, 5)
    assert (want_s != S.NONE).sum() >= 10
    assert np.array_equal(disp.cpu().numpy(), want_d) and np.array_equal(status.cpu().numpy(), want_s)
    assert disp.dtype == torch.int32 and status.dtype == torch.uint8 and tuple(disp.shape) == (1, 64)


def test_feature_tracks_with_integer_q8_is_todays_and_refined_follows_the_formula(golden):
    fe, res, images_d, disp, status, h = golden
    ids0, feats0, n0 = fe.feature_tracks(res)
    d0 = torch.from_numpy(S.integer_disparity_q8(h["sidx"], h["keys"], h["cnt"], 128)).cuda()
    ids1, feats1, n1 = fe.feature_tracks(res, disparity=d0)
    assert n0 == n1 and torch.equal(ids0, ids1)
    assert np.array_equal(feats0.cpu().numpy().view(np.uint64), feats1.cpu().numpy().view(np.uint64))     # bit for bit
    ids2, feats2, n2 = fe.feature_tracks(res, disparity=disp)
    assert n0 == n2 and torch.equal(ids0, ids2)
    f0, f2 = feats0.cpu().numpy(), feats2.cpu().numpy()
    assert np.array_equal(f0[..., [0, 1, 3]].view(np.uint64), f2[..., [0, 1, 3]].copy().view(np.uint64))
    live = ids0.cpu().numpy() >= 0
    assert live.sum() >= 10
    pos = h["keys"][0].astype(np.int64) & S.T.POS_MASK
    want = S.u1((pos % 128)[None, :], disp.cpu().numpy(), 128)
    assert np.array_equal(f2[..., 2][live].view(np.uint64), want[live].view(np.uint64))
    assert np.array_equal(f2[..., 2][~live], f0[..., 2][~live])
    assert (f2[..., 2][live] != f0[..., 2][live]).any()
    msgs = fe.camera_measurements(res, disparity=disp)
    assert [ft.u1 for ft in msgs[0].features] == f2[0, live[0], 2].tolist()


def run_q8(t, disp_q8, **kw):
    """TL.run_gpu for vus_stereo_pair_pose_q8 (disp_q8 None: a NULL pointer)."""
    from visual_underwater_slam_amd import _lib as L
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = dict(threshold_px=R.THRESHOLD, n_hyp=R.N_HYP, seed=R.SEED, refine_iters=R.REFINE)
    p.update(kw)
    mt, pa, pb = d(t["match_idx"].astype(np.int32)), d(t["pair_a"].astype(np.int32)), d(t["pair_b"].astype(np.int32))
    st, keys, cnt = d(t["stereo_idx"].astype(np.int32)), d(t["kp_keys"].view(np.int32)), d(t["kp_count"].astype(np.int32))
    q8 = None if disp_q8 is None else d(np.asarray(disp_q8, np.int32))
    P, K = t["match_idx"].shape
    out = torch.full((P, K), TL.SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.full((P, 6), TL.SENTINEL, dtype=torch.int32, device="cuda")
    T = torch.full((P, 12), TL.FSENT, dtype=torch.float64, device="cuda")
    JtJ = torch.full((P, 36), TL.FSENT, dtype=torch.float64, device="cuda")
    rss = torch.full((P,), TL.FSENT, dtype=torch.float64, device="cuda")
    cam = np.ascontiguousarray(t["cam"], np.float64)
    L.call("vus_stereo_pair_pose_q8", mt.data_ptr(), pa.data_ptr(), pb.data_ptr(), st.data_ptr(), keys.data_ptr(), cnt.data_ptr(),
           len(t["stereo_idx"]), P, K, t["H"], t["W"], cam.ctypes.data, float(p["threshold_px"]), int(p["n_hyp"]), int(p["seed"]),
           int(p["refine_iters"]), None if q8 is None else q8.data_ptr(), T.data_ptr(), JtJ.data_ptr(), rss.data_ptr(),
           out.data_ptr(), info.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    return dict(T_ab=T.cpu().numpy(), JtJ=JtJ.cpu().numpy(), rss=rss.cpu().numpy(), match_idx_out=out.cpu().numpy(),
                info=info.cpu().numpy())


@pytest.mark.parametrize("name", ["planted_kp257", "bad_tables"])
def test_pair_pose_q8_with_null_and_with_integer_q8_gives_the_bits_of_pair_pose(gpu, name):
    t, ref = R.case(name)
    base = TL.run_gpu(t)
    TL.compare(base, ref, name)
    d0 = S.integer_disparity_q8(t["stereo_idx"], t["kp_keys"], t["kp_count"], t["W"])
    for what, got in (("NULL", run_q8(t, None)), ("256 d0", run_q8(t, d0))):
        for k in base:
            assert np.array_equal(base[k], got[k]), (name, what, k)


def fractional(t, seed):
    """256 d0 plus a planted fraction in [-128, 128) on every matched slot."""
    d0 = S.integer_disparity_q8(t["stereo_idx"], t["kp_keys"], t["kp_count"], t["W"])
    frac = np.random.default_rng(seed).integers(-128, 128, d0.shape).astype(np.int32)
    return np.where(d0 != 0, d0 + frac, 0).astype(np.int32)


@pytest.mark.parametrize("name", ["planted_kp257", "batch9"])
def test_pair_pose_q8_with_fractional_disparities_equals_the_reference(gpu, name):
    t = R.tables(name)
    q8 = fractional(t, 77)
    mg = R.Margins()
    ref = S.stereo_pair_pose_q8(t, q8, R.THRESHOLD, R.N_HYP, R.SEED, R.REFINE, mg)
    assert mg.safe(), mg                                     # the fixture is certified: no decision within rounding of its bound
    got = run_q8(t, q8)
    TL.compare(got, ref, (name, "q8"))
    assert (ref["info"][:, 4] == 0).all()
    whole = TL.run_gpu(t)
    assert not np.array_equal(whole["T_ab"], got["T_ab"])    # the fractions do enter the depths
