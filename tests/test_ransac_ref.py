"""The numpy statement of vus_two_point_ransac (tests/ransac_ref.py) against planted truth, its tie-break and `info`
on hand-built tables, the edges its adversarial tables must really contain, and the entry point's host-side argument
checks (no GPU needed: validation precedes any launch)."""
import ctypes

import numpy as np
import pytest

import ransac_ref as R
from visual_underwater_slam_amd import synth

N_PAIRS = 8      # pairs p per planted case (each p draws other samples and another scene)


@pytest.mark.parametrize("name", list(R.PLANTED))
def test_reference_separates_planted_matches(name):
    """At 1280 x 720, threshold 3 px, seed synth.SEED: >= 98 % of the true matches survive and >= 90 % of the wrong ones
    are rejected, for every pair.  (A prototype of the same arithmetic gave minima of 99.7 % and 95.8 % over 20 pairs
    per case: the bounds are caps with room to spare, not measurements.)"""
    n_true, n_wrong, n_hyp, t, w = R.PLANTED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    cam = R.default_cam(R.PLANTED_H, R.PLANTED_W)
    for p in range(N_PAIRS):
        x1, y1, x2, y2, truth, R9 = R.planted_pair(rng, n_true, n_wrong, t, w, R.PLANTED_H, R.PLANTED_W)
        keep, best, n_static, counts = R.pair_ransac(x1, y1, x2, y2, R9, cam, R.PLANTED_THRESHOLD, n_hyp, synth.SEED, p)
        kept, rejected = keep[truth].mean(), 1.0 - keep[~truth].mean()
        print(f"{name} p={p}: kept {kept:.4f} of the true, rejected {rejected:.4f} of the wrong, best={best}")
        assert best >= 0 and len(counts) == n_hyp
        assert kept >= 0.98, (name, p, kept)
        assert rejected >= 0.90, (name, p, rejected)
        if name == "pure_rotation":       # every true match is `static`; the model only has to leave them alone
            assert n_static >= n_true


def test_mix_is_the_hash_of_synth():
    for v in (0, 1, 0xFFFFFFFF, 20261004, 0x9E3779B9):
        assert R.mix(v) == synth._mix32_scalar(v) == int(synth._mix32(np.array([v], np.int64))[0])


def _two_match_table():
    """Two true matches of a sideways translation, R = I: n = 2, so hypotheses 0 and 1 both sample the pair {0, 1}."""
    H, W = 480, 640
    cam = R.default_cam(H, W)
    rng = np.random.default_rng(5)
    x1, y1, x2, y2, truth, R9 = R.planted_pair(rng, 2, 0, (0.3, 0.0, 0.0), (0, 0, 0), H, W)
    return H, W, cam, (x1, y1, x2, y2), R9


def test_tie_goes_to_the_lowest_hypothesis():
    H, W, cam, m, R9 = _two_match_table()
    keep, best, n_static, counts = R.pair_ransac(*m, R9, cam, 3.0, 8, synth.SEED, 0)
    assert n_static == 0                       # they moved by tens of pixels
    assert counts.tolist() == [2] * 8          # every hypothesis is the same pair of samples, both on their own line
    assert best == 0 and keep.tolist() == [True, True]
    # and through the table form, with the slots in between empty: info = (n, surviving, best, static)
    tb = R.tables_from_pairs(np.random.default_rng(6), [m], 16, H, W)
    out, info = R.two_point_ransac(tb["track_idx"], tb["kp_keys"], tb["kp_count"], H, W, R9[None], cam, 3.0, 8, synth.SEED)
    assert info.tolist() == [[2, 2, 0, 0]]
    assert np.array_equal(out, tb["track_idx"])


def test_best_is_the_first_maximum_and_a_sample_behind_the_camera_disqualifies():
    t, (out, info) = R.case("behind", n_hyp=64)
    P = len(info)
    seen_minus = False
    for p in range(P):
        nl = min(int(t["kp_count"][2 * p]), t["track_idx"].shape[1])
        src = np.nonzero(t["track_idx"][p, :nl] >= 0)[0]
        x1, y1 = R.decode(t["kp_keys"][2 * p, src], t["W"])
        x2, y2 = R.decode(t["kp_keys"][2 * p + 2, t["track_idx"][p, src]], t["W"])
        keep, best, n_static, counts = R.pair_ransac(x1, y1, x2, y2, t["rot"][p], t["cam"], 3.0, 64, 20261004, p)
        seen_minus |= bool((counts == -1).any())
        if counts.max() >= 0:
            assert best == int(np.argmax(counts)) and info[p, 2] == best
        else:
            assert best == -1 and info[p, 2] == -1
    assert seen_minus
    assert info[2].tolist() == [120, 0, -1, 0] and (out[2] == -1).all()       # every ray behind: nothing is `front`
    assert 0 < info[0, 1] < 120 and info[0, 2] >= 0


def test_adversarial_tables_contain_their_edges():
    t, (out, info) = R.case("few_matches")
    assert info[:, 0].tolist() == [0, 1, 2, 3, 2, 3]
    assert info[0].tolist() == [0, 0, -1, 0] and info[1, 2] == -1 and info[1, 1] == 1      # n < 2: no model, front survives
    assert (info[2:, 2] >= 0).all()
    t, (out, info) = R.case("all_static_identity")
    assert np.array_equal(info[:, 0], info[:, 3]) and np.array_equal(info[:, 0], info[:, 1]) and (info[:, 2] == 0).all()
    assert np.array_equal(out, t["track_idx"])
    t, (out, info) = R.case("all_outliers")
    assert (info[:, 1] < 0.25 * info[:, 0]).all() and (info[:, 1] >= 2).all()              # the two samples fit themselves
    t, (out, info) = R.case("make_tables")
    K = t["track_idx"].shape[1]
    cnt, trk = t["kp_count"], t["track_idx"]
    assert (cnt[0::2] > K).any() and (cnt[0::2] < 0).any() and (cnt[0::2] == 0).any()
    assert (trk >= K).any() and (trk < -1).any()
    targets = [trk[p][(trk[p] >= 0) & (trk[p] < K)] for p in range(len(trk))]
    assert any(len(np.unique(v)) < len(v) for v in targets)                                  # colliding targets
    assert info[3].tolist()[:2] == [0, 0] and info[4].tolist()[:2] == [0, 0]                 # the negative count: no target / no source
    assert (out[3] == -1).all() and (out[4] == -1).all()
    assert (info[:3, 0] > 50).all() and (info[:, 1] <= info[:, 0]).all()
    # survivors keep their index, everything else is -1
    live = out >= 0
    assert np.array_equal(out[live], trk[live]) and (out[~live] == -1).all()


def test_large_case_crosses_the_lds_residency_switch():
    t, (out, info) = R.case("large")
    assert 3900 <= info[0, 0] <= 4100 and info[0, 0] > 2000          # VUS_RANSAC_LDS_MATCHES of include/vus_ransac.h
    assert info[0, 2] >= 0 and 0.6 * info[0, 0] <= info[0, 1] < info[0, 0]


def test_host_side_argument_checks_need_no_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    assert "vus_two_point_ransac" in L.SIGNATURES
    p8 = ctypes.c_void_p(8)                       # never dereferenced: every call below fails validation first
    cam = np.array([1218.0, 1218.4, 645.9, 374.3])
    good = dict(track=p8, keys=p8, count=p8, F=3, K=2000, H=720, W=1280, rot=p8, cam=cam.ctypes.data, thr=3.0, hyp=256,
                seed=1, out=p8, info=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_two_point_ransac(a["track"], a["keys"], a["count"], a["F"], a["K"], a["H"], a["W"], a["rot"], a["cam"],
                                      a["thr"], a["hyp"], a["seed"], a["out"], a["info"], None)
        return rc, lib.vus_last_error()

    for name in ("track", "keys", "count", "rot", "cam", "out", "info"):
        rc, msg = call(**{name: None})
        assert rc == -1 and b"null" in msg, name
    for kw, word in ((dict(F=1), b"n_frames"), (dict(F=0), b"n_frames"), (dict(K=0), b"max_kp"), (dict(K=8193), b"max_kp"),
                     (dict(hyp=0), b"n_hyp"), (dict(hyp=4097), b"n_hyp"), (dict(thr=0.0), b"threshold_px"),
                     (dict(thr=-3.0), b"threshold_px"), (dict(thr=float("nan")), b"threshold_px"),
                     (dict(thr=float("inf")), b"threshold_px")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for slot in (0, 1):
            c = cam.copy()
            c[slot] = bad
            rc, msg = call(cam=c.ctypes.data)
            assert rc == -1 and b"focal" in msg, (bad, slot, msg)
    assert lib.vus_abi_version() == 1
