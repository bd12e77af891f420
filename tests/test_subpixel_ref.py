"""The numpy statement of vus_stereo_refine (tests/subpixel_ref.py) does what include/vus_subpixel.h says on inputs whose
answer is known, and both new entry points are exported, bound and refuse every invalid argument on the host, before any
launch, with a message that names it (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

import subpixel_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(H, W, pts):
    """One frame whose left keypoint i = (xl, yl) is matched to right keypoint i = (xr, yr): pts rows (xl, yl, xr, yr)."""
    pts = np.asarray(pts, np.int64).reshape(-1, 4)
    n = len(pts)
    keys = np.zeros((2, n), np.uint32)
    keys[0] = (7 << 24) | (pts[:, 1] * W + pts[:, 0])
    keys[1] = (9 << 24) | (pts[:, 3] * W + pts[:, 2])
    return np.arange(n, dtype=np.int32)[None, :], keys, np.array([n, n], np.int32)


def test_whole_pixel_shift_is_found_with_q_zero():
    """right = left moved k columns (a true disparity of k): whatever integer start d0 within the search, s* = d0 - k.
    On white noise the cost at s* is 0 and its two neighbours are unequal sums of unrelated pixels, so the output is
    256 k - q with the q of those two costs; on a horizontal ramp the cost is a true V, the neighbours are equal, q = 0 and
    the output is 256 k exactly."""
    rng = np.random.default_rng(1)
    H, W = 48, 96
    wide = rng.integers(0, 256, (H, W + 16), dtype=np.uint8)
    for k in (0, 3, 7):
        left, right = wide[:, :W], wide[:, k:k + W]                  # right[x] = left[x + k]: xr = xl - k
        img = np.stack([left, right])
        pts = []
        for d0 in range(k - 4, k + 5):
            xl = 40 + d0
            pts.append((xl, 20, xl - d0, 22))                        # the right keypoint's row is not used
        sidx, keys, cnt = tables(H, W, pts)
        disp, status, cost = S.refine(img, W, sidx, keys, cnt, 5, 5, return_costs=True)
        c = cost[0]
        for n, d0 in enumerate(range(k - 4, k + 5)):
            s = d0 - k
            assert c[n, s + 5] == 0 and status[0, n] == S.OK
            q = S.fit_q(c[n, s + 4], 0, c[n, s + 6])
            assert disp[0, n] == 256 * k - q and abs(int(q)) <= 128
    # a horizontal ramp has equal neighbours: q = 0 exactly
    ramp = np.broadcast_to((2 * np.arange(W + 16)).astype(np.uint8), (H, W + 16))
    img = np.stack([ramp[:, :W], ramp[:, 4:4 + W]])
    sidx, keys, cnt = tables(H, W, [(40, 20, 34, 20), (50, 10, 47, 10)])      # d0 = 6 and 3, truth 4
    disp, status = S.refine(img, W, sidx, keys, cnt, 3, 4)
    assert disp.tolist() == [[1024, 1024]] and status.tolist() == [[S.OK, S.OK]]


def test_floor_division_and_the_range_of_q():
    for c0 in range(0, 7):
        for cm in range(c0, c0 + 9):
            for cp in range(c0, c0 + 9):
                q = int(S.fit_q(cm, c0, cp))
                m = max(cm, cp) - c0
                if m == 0:
                    assert q == 0
                    continue
                num = 256 * (cm - cp) + m
                assert q == np.floor(num / (2 * m)) and 2 * m * q <= num < 2 * m * (q + 1)      # floor, not truncation
                assert -128 <= q <= 128
    assert int(S.fit_q(0, 0, 5)) == -128 and int(S.fit_q(5, 0, 0)) == 128 and int(S.fit_q(5, 0, 5)) == 0
    assert int(S.fit_q(1, 0, 3)) == -85            # (-512 + 3) / 6 = -84.83: floor -85, truncation would give -84
    q = S.fit_q(np.array([57375, 0, 3]), np.array([0, 0, 3]), np.array([0, 57375, 3]))
    assert q.tolist() == [128, -128, 0]


def test_flat_image_ends_at_the_edge():
    H, W = 40, 72
    img = np.full((2, H, W), 93, np.uint8)
    rng = np.random.default_rng(2)
    pts = [(int(x), int(y), int(x) - int(d), int(y)) for x, y, d in zip(rng.integers(20, W, 30), rng.integers(0, H, 30), rng.integers(0, 20, 30))]
    sidx, keys, cnt = tables(H, W, pts)
    disp, status = S.refine(img, W, sidx, keys, cnt, 5, 5)
    assert (status == S.EDGE).all() and disp[0].tolist() == [256 * (p[0] - p[2]) for p in pts]


def test_windows_are_clamped_at_the_four_corners():
    """Against a direct loop over an explicitly padded image (np.pad mode="edge" is the replicate border)."""
    rng = np.random.default_rng(3)
    H, W, hw, sr = 40, 72, 7, 8
    img = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    pts = [(0, 0, 0, 0), (W - 1, 0, W - 1, 0), (0, H - 1, 0, H - 1), (W - 1, H - 1, W - 1, H - 1), (3, 2, 0, 2), (W - 1, H - 2, W - 9, H - 2)]
    sidx, keys, cnt = tables(H, W, pts)
    _, _, cost = S.refine(img, W, sidx, keys, cnt, hw, sr, return_costs=True)
    pad = hw + sr
    P = np.pad(img.astype(np.int64), ((0, 0), (pad, pad), (pad, pad)), mode="edge")
    for n, (xl, yl, xr, _) in enumerate(pts):
        for k, s in enumerate(range(-sr, sr + 1)):
            lw = P[0, pad + yl - hw:pad + yl + hw + 1, pad + xl - hw:pad + xl + hw + 1]
            rw = P[1, pad + yl - hw:pad + yl + hw + 1, pad + xr + s - hw:pad + xr + s + hw + 1]
            assert cost[0][n, k] == np.abs(lw - rw).sum(), (n, s)


def test_unmatched_slots_and_the_u1_formula():
    H, W = 40, 72
    img = np.random.default_rng(4).integers(0, 256, (2, H, W), dtype=np.uint8)
    sidx = np.array([[0, -1, 5, 2, 2 ** 31 - 1, -7, 1]], np.int32)
    keys = np.random.default_rng(5).integers(0, H * W, (2, 7)).astype(np.uint32)
    disp, status = S.refine(img, W, sidx, keys, np.array([6, 3], np.int32), 2, 2)
    assert status[0, [1, 2, 4, 5, 6]].tolist() == [S.NONE] * 5 and disp[0, [1, 2, 4, 5, 6]].tolist() == [0] * 5
    assert (status[0, [0, 3]] != S.NONE).all()
    disp, status = S.refine(img, W, sidx, keys, np.array([-1, 99], np.int32), 2, 2)
    assert (status == S.NONE).all() and (disp == 0).all()
    # u1: integer disparities reproduce 2 x / W - 1 bit for bit, fractions are exact in f64
    xl, xr = np.arange(0, 640), (np.arange(0, 640) * 7) % 640
    assert np.array_equal(S.u1(xl, 256 * (xl - xr), 640), 2.0 * xr.astype(np.float64) / 640.0 - 1.0)
    assert S.u1(100, 256 * 10 + 64, 640) == 2.0 * 89.75 / 640.0 - 1.0


def test_symbols_are_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    sub = strip(open(os.path.join(ROOT, "include", "vus_subpixel.h")).read())
    loop = strip(open(os.path.join(ROOT, "include", "vus_loop.h")).read())
    own = strip(open(os.path.join(ROOT, "include", "vus.h")).read())
    assert '#include "vus_subpixel.h"' in own and "vus_stereo_refine" not in own and "vus_stereo_pair_pose_q8" not in own
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, hdr, n in (("vus_stereo_refine", sub, 14), ("vus_stereo_pair_pose_q8", loop, 23)):
        assert hasattr(lib, name)
        assert len(L.SIGNATURES[name]) == n
        assert len(re.search(name + r"\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")) == n
        assert getattr(L.load(), name).restype is ctypes.c_int
    assert L.load().vus_abi_version() == 1


def test_stereo_refine_rejects_invalid_arguments_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                       # never dereferenced: every call below fails validation first
    good = dict(img=p8, F=2, H=360, W=640, pitch=640, stereo_idx=p8, kp_keys=p8, kp_count=p8, K=2000, hw=5, sr=5, disp_q8=p8,
                status=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_stereo_refine(a["img"], a["F"], a["H"], a["W"], a["pitch"], a["stereo_idx"], a["kp_keys"], a["kp_count"],
                                   a["K"], a["hw"], a["sr"], a["disp_q8"], a["status"], None)
        return rc, lib.vus_last_error()

    for name in ("img", "stereo_idx", "kp_keys", "kp_count", "disp_q8", "status"):
        rc, msg = call(**{name: None})
        assert rc == -1 and name.encode() in msg and b"null" in msg, (name, msg)
    for kw, word in ((dict(F=0), b"n_frames"), (dict(F=-2), b"n_frames"), (dict(H=0), b"H="), (dict(W=0, pitch=0), b"W="),
                     (dict(pitch=639), b"pitch"), (dict(K=0), b"max_kp"), (dict(K=65536), b"max_kp"), (dict(hw=0), b"half_win"),
                     (dict(hw=8), b"half_win"), (dict(sr=0), b"search"), (dict(sr=9), b"search"), (dict(sr=-1), b"search"),
                     (dict(F=40000, K=65535), b"n_frames")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)


def test_pair_pose_q8_rejects_invalid_arguments_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)
    cam = np.array([609.0, 609.2, 322.97, 187.1, 0.063])
    good = dict(match=p8, pa=p8, pb=p8, stereo=p8, keys=p8, count=p8, F=4, P=2, K=2000, H=360, W=640, cam=cam.ctypes.data,
                thr=2.0, hyp=256, seed=1, refine=10, q8=p8, T=p8, JtJ=p8, rss=p8, out=p8, info=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_stereo_pair_pose_q8(a["match"], a["pa"], a["pb"], a["stereo"], a["keys"], a["count"], a["F"], a["P"], a["K"],
                                         a["H"], a["W"], a["cam"], a["thr"], a["hyp"], a["seed"], a["refine"], a["q8"], a["T"],
                                         a["JtJ"], a["rss"], a["out"], a["info"], None)
        return rc, lib.vus_last_error()

    for q8 in (p8, None):                         # disp_q8 itself may be null: integer disparities
        for name in ("match", "pa", "pb", "stereo", "keys", "count", "cam", "T", "JtJ", "rss", "out", "info"):
            rc, msg = call(q8=q8, **{name: None})
            assert rc == -1 and b"null" in msg, name
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(P=0), b"n_pairs"), (dict(F=0), b"n_frames"), (dict(K=0), b"max_kp"), (dict(K=4097), b"max_kp"),
                     (dict(hyp=0), b"n_hyp"), (dict(hyp=4097), b"n_hyp"), (dict(refine=-1), b"refine_iters"),
                     (dict(refine=65), b"refine_iters"), (dict(H=0), b"H="), (dict(W=0), b"W="), (dict(thr=0.0), b"threshold_px"),
                     (dict(thr=nan), b"threshold_px"), (dict(thr=inf), b"threshold_px")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for bad in (0.0, -1.0, nan, inf):
        for slot, word in ((0, b"focal"), (1, b"focal"), (4, b"baseline")):
            c = cam.copy()
            c[slot] = bad
            rc, msg = call(cam=c.ctypes.data)
            assert rc == -1 and word in msg, (bad, slot, msg)
