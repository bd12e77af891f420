"""tests/track_ref.py pinned against the C oracle on the CPU: the plain restatement of the id propagation, factor
emission, initial residual, mutual-match filter and pyramid append equals the oracle on every generated case --
integers exactly, floats bit for bit -- and every case contains the edges it was generated for.  Also the filtering
half of BatchSequence.gate_factors, with the oracle standing in for the residual kernel."""
import ctypes

import numpy as np
import pytest

import track_ref as R


def _oracle_emit(oracle, e, n_ids, first_frame):
    """vus_emit_stereo_factors_cpu with every output pre-filled: the raw buffers, not sliced to the count."""
    ids = np.ascontiguousarray(e["ids"], np.int64)
    F, K = ids.shape
    p = oracle._p
    out = dict(frame_base=np.full(F + 1, -77, np.int32), count=np.full(1, -77, np.int32),
               obs_frame=np.full(F * K + 1, -77, np.int32), obs_id=np.full(F * K + 1, -77, np.int64),
               obs_meas=np.full((F * K + 1, 3), -77.0), lm_first=np.full(n_ids + 1, -77, np.int64),
               lm_point=np.zeros((n_ids + 1, 3)))
    rc = oracle.lib().vus_emit_stereo_factors_cpu(p(ids), p(e["feat"]), p(e["Rt"]), p(e["cam"]), F, K, int(first_frame),
                                                  ctypes.c_longlong(n_ids), p(out["frame_base"]), p(out["count"]),
                                                  p(out["obs_frame"]), p(out["obs_id"]), p(out["obs_meas"]),
                                                  p(out["lm_first"]), p(out["lm_point"]))
    assert rc == 0
    return out


def _oracle_track(oracle, t):
    F, K = t["stereo_idx"].shape
    if F:
        return oracle.track_ids(t["stereo_idx"], t["track_idx"], t["kp_keys"], t["kp_count"], t["H"], t["W"])
    p = oracle._p                       # no frame: the entry point wants non-null buffers all the same
    pad, ids, feat, n = np.zeros((2, K), np.int32), np.zeros((1, K), np.int64), np.zeros((1, K, 4)), np.full(1, -5, np.int64)
    assert oracle.lib().vus_track_ids_cpu(p(pad), None, p(pad), p(pad), 0, K, t["H"], t["W"], p(ids), p(feat), p(n)) == 0
    return ids[:0], feat[:0], int(n[0])


def check_emission(got, ref, n_ids):
    """Raw output buffers (one spare row each, pre-filled with -77 / zero points) against the reference's factors."""
    n = len(ref["obs_frame"])
    assert int(got["count"][0]) == n
    assert np.array_equal(got["frame_base"], ref["frame_base"])
    assert np.array_equal(got["obs_frame"][:n], ref["obs_frame"]) and np.array_equal(got["obs_id"][:n], ref["obs_id"])
    assert R.same_bits(got["obs_meas"][:n], ref["obs_meas"])
    assert np.array_equal(got["lm_first"][:n_ids], ref["lm_first"])
    assert R.same_bits(got["lm_point"][:n_ids], ref["lm_point"])          # never-seen ids keep the caller's zeros
    # rows at or above the count, and the spare landmark row, are untouched
    assert (got["obs_frame"][n:] == -77).all() and (got["obs_id"][n:] == -77).all() and (got["obs_meas"][n:] == -77.0).all()
    assert got["lm_first"][n_ids] == -77 and (got["lm_point"][n_ids] == 0).all()


def assert_track_case_contents(name, t, ids, n_ids, carried):
    """The edges a case was generated for are really in it (counted from the tables and the reference's output)."""
    p = R.track_properties(t, ids, carried)
    F, K = ids.shape
    if name == "adversarial":
        assert p["collisions"] >= 50 and p["collisions_idless_lowest"] >= 10, p
        assert p["track_stale"] >= 10 and p["track_oob"] >= 10 and p["track_negative"] >= 5 and p["stereo_stale"] >= 10, p
        assert p["over_left"] >= 1 and p["over_right"] >= 1 and p["negative"] >= 1 and p["lost_tracks"] >= 10, p
        published = [set(ids[f][ids[f] >= 0].tolist()) for f in range(F)]
        # frame 3 has no left keypoints: nothing is published there and no id crosses it, so numbering restarts
        assert not published[3] and set().union(*published[:3]).isdisjoint(set().union(*published[4:]))
        assert min(published[4]) == max(set().union(*published[:3])) + 1 and (carried[3] < 0).all()
        # frame 5 has no right keypoints: nothing is published, the left keypoints carry their ids on (include/vus.h)
        assert not published[5] and (carried[5] >= 0).any() and published[4] & published[6]
        # frame 7's left count is negative: an empty list
        assert not published[7] and (carried[7] < 0).all() and published[8]
        # ids are issued once, in publication order: the first sightings are 0, 1, 2, ... in frame-major slot order
        flat = ids[ids >= 0]
        _, first_at = np.unique(flat, return_index=True)
        assert np.array_equal(flat[np.sort(first_at)], np.arange(n_ids))
    if name == "frames40":
        assert p["long_tracks"] >= 1 and (ids[:, 0] == 0).all(), p
    if name.startswith("max_kp") and K >= 63:
        assert p["collisions"] >= 10 and p["over_left"] >= 1 and p["over_right"] >= 1 and p["lost_tracks"] >= 1, p
    if name == "full_lists":
        assert (t["kp_count"] == K).all()
    if name == "frames0":
        assert n_ids == 0


@pytest.mark.parametrize("name", list(R.TRACK_CASES))
def test_track_ids_reference_equals_oracle(oracle, name):
    t, (ids, feat, n_ids, carried) = R.track_case(name)
    F, K = ids.shape
    oids, ofeat, on = _oracle_track(oracle, t)
    assert on == n_ids
    assert np.array_equal(oids, ids)
    assert R.same_bits(ofeat, feat)
    assert (feat[ids < 0] == 0).all()
    assert_track_case_contents(name, t, ids, n_ids, carried)


def assert_emit_case_contents(name, e, n_ids, first_frame, ref):
    p = R.emission_properties(e, n_ids, first_frame, ref)
    F, K = e["ids"].shape
    assert p["count"] == len(ref["obs_frame"])
    if K >= 40 and name != "all_empty":
        assert p["id_eq_n_ids"] >= 1 and p["id_above"] >= 1 and p["id_negative"] >= 1, p
    if name.startswith("frames") and F >= 1023:
        assert p["empty_start"] and p["empty_middle"] and p["empty_end"] and p["zero_disparity"] >= 20, p
        assert p["negative_disparity"] >= 20 and p["duplicates"] >= 100, p
    if name == "first3":
        assert p["only_before_first"] >= 1 and p["never_seen"] >= p["only_before_first"] and p["duplicates"] >= 1, p
        assert p["empty_start"] and p["empty_middle"] and p["empty_end"], p
    if name in ("first6", "first8", "all_empty", "n_ids0"):
        assert p["count"] == 0 and (ref["lm_first"] == -1).all()
    if name == "n_ids1":
        assert p["count"] >= 6 and ref["lm_first"][0] == 1 * K + 0          # id 0 in slot 0 of keyframe 1: first sighting
    if name == "first1":
        # an id twice in one keyframe: both factors, and the first slot is the first sighting
        f = 1
        lid = int(e["ids"][f, 0])
        assert e["ids"][f, K - 1] == lid and ref["lm_first"][lid] == f * K
        assert ((ref["obs_frame"] == f) & (ref["obs_id"] == lid)).sum() >= 2


@pytest.mark.parametrize("name", list(R.EMIT_CASES))
def test_emission_reference_equals_oracle(oracle, name):
    e, n_ids, first_frame, ref = R.emit_case(name)
    check_emission(_oracle_emit(oracle, e, n_ids, first_frame), ref, n_ids)
    assert_emit_case_contents(name, e, n_ids, first_frame, ref)


def test_track_ids_feed_the_emission_like_the_oracle_chain(oracle):
    """The two stages chained on the adversarial tables, first_frame 1 as batch_create has it."""
    t, (ids, feat, n_ids, _) = R.track_case("adversarial")
    Rt = R.random_poses(np.random.default_rng(3), ids.shape[0])
    e = dict(ids=ids, feat=feat, Rt=Rt, cam=R.CAM)
    ref = R.emit_stereo_factors(ids, feat, Rt, R.CAM, n_ids, 1)
    check_emission(_oracle_emit(oracle, e, n_ids, 1), ref, n_ids)
    assert len(ref["obs_frame"]) == (ids[1:] >= 0).sum() and (ref["lm_first"] < 0).sum() >= 1


def assert_residual_case_contents(n, c, resid):
    p = R.residual_properties(c, resid)
    if n >= 255:
        assert p["inf_rows"] >= 20 and p["on_plane"] >= 10 and p["nonfinite_points"] >= 15 and p["finite_rows"] >= 50, p
    assert p["mixed_rows"] == 0, p          # the cheirality case sets all three components


@pytest.mark.parametrize("n", R.RESIDUAL_N)
def test_residual_reference_equals_oracle(oracle, n):
    c, resid = R.residual_case(n)
    got = oracle.stereo_initial_residuals(c["Rt"], c["K6"], c["lm_point"], c["obs_frame"], c["obs_id"], c["obs_meas"])
    assert np.array_equal(np.isposinf(got).all(1), np.isposinf(resid).all(1))
    assert R.same_bits(got, resid)
    assert_residual_case_contents(n, c, resid)


@pytest.mark.parametrize("P,K", R.CROSS_CHECK_CASES)
def test_cross_check_reference_equals_oracle(oracle, P, K):
    fwd, bwd = R.make_cross_check(10 * K + P, P, K)
    want = R.cross_check(fwd, bwd)
    if P:
        assert np.array_equal(oracle.cross_check(fwd, bwd), want)
    if P * K >= 257:
        kept = want >= 0
        assert kept.sum() >= 50 and ((fwd >= 0) & (fwd < K) & ~kept).sum() >= 50 and (fwd >= K).sum() >= 1


def pyramid_reference(levels, fill):
    m = R.new_merged(len(R.PYR_COUNTS), R.PYR_MAX_KP, fill)
    H0, W0 = R.PYR_SIZES[0]
    counts = []
    for lv, (keys, cnt, desc, ang, Hl, Wl) in enumerate(levels):
        R.pyramid_append(keys, cnt, desc, ang, Hl, Wl, lv, H0, W0, m)
        counts.append(m["kp_count"].copy())
    return m, np.array(counts)


def assert_pyramid_case_contents(levels, counts):
    """counts [level, image]: the merged count after each level."""
    before = np.vstack([np.zeros_like(counts[:1]), counts[:-1]])
    asked = np.array([lv[1] for lv in levels])
    room = R.PYR_MAX_KP - before
    assert (asked == 0).any() and (asked > R.PYR_LVL_MAX_KP).any()                 # an empty level, one above its capacity
    assert ((asked == room) & (room > 0)).any() and (asked > room).any()           # exactly the quota, and above it
    assert ((room == 0) & (asked > 0) & (counts == before)).any()                  # a full list: nothing appended
    assert (counts[-1] < R.PYR_MAX_KP).any()


@pytest.mark.parametrize("n_levels", [2, 3, 4])
def test_pyramid_append_reference_equals_oracle(oracle, n_levels):
    """Level 0 and one, two or three appended levels."""
    levels = R.make_pyramid_levels(n_levels, n_levels)
    want, counts = pyramid_reference(levels, 0x5A)
    got = R.new_merged(len(R.PYR_COUNTS), R.PYR_MAX_KP, 0x5A)
    H0, W0 = R.PYR_SIZES[0]
    for lv, (keys, cnt, desc, ang, Hl, Wl) in enumerate(levels):
        oracle.pyramid_append(keys, cnt, desc, ang, Hl, Wl, lv, H0, W0, got)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert_pyramid_case_contents(levels, counts)
    tail = np.arange(R.PYR_MAX_KP)[None, :] >= want["kp_count"][:, None]
    assert (want["kp_keys"][tail] == 0xFFFFFFFF).all() and (want["kp_level"][tail] == 0x5A).all()


# ----------------------------------------------------------------------------------------------------------------------
# the gate: the reference's rule, and the torch filtering of BatchSequence.gate_factors around the residual call

def gate_case(oracle):
    """(factors of emission case `dense`, Rt, the oracle's residuals, the gates)."""
    e, n_ids, first_frame, ref = R.emit_case("dense")
    resid = oracle.stereo_initial_residuals(e["Rt"], R.K6, ref["lm_point"], ref["obs_frame"], ref["obs_id"], ref["obs_meas"])
    return ref, e["Rt"], resid, R.gate_thresholds(resid, ref["obs_id"])


def assert_gate_case_contents(ref, resid, gates):
    assert set(gates) == {"all", "finite", "none", "first_dropped"}
    m = np.abs(resid).max(1)
    g = gates["first_dropped"]
    keep, _, kid, _, first = R.gate(resid, g, ref["obs_frame"], ref["obs_id"], ref["obs_meas"], ref["lm_first"])
    assert (m == g).any() and keep[m == g].all()                                   # a residual exactly on the gate is kept
    assert 0 < keep.sum() < len(keep)
    lost = (ref["lm_first"] >= 0) & (first < 0)
    assert lost.any()                                                              # a landmark lost every factor
    order = {}
    for a, lid in enumerate(ref["obs_id"]):
        order.setdefault(int(lid), []).append(a)
    assert any(not keep[v[0]] and keep[v[1:]].any() for v in order.values())       # first sighting gone, a later one kept
    assert np.isposinf(resid).all(1).sum() >= 20
    k_all = R.gate(resid, gates["all"], ref["obs_frame"], ref["obs_id"], ref["obs_meas"], ref["lm_first"])
    assert k_all[0].sum() == (~np.isnan(resid).any(1)).sum() >= len(keep) - 20
    k_none = R.gate(resid, gates["none"], ref["obs_frame"], ref["obs_id"], ref["obs_meas"], ref["lm_first"])
    assert not k_none[0].any() and (k_none[4] == -1).all()


def check_gate_output(out, want, resid):
    """gate_factors' dict against track_ref.gate's tuple."""
    keep, of, oi, om, first = want
    assert np.array_equal(out["gate_keep"].cpu().numpy(), keep)
    assert np.array_equal(out["obs_frame"].cpu().numpy(), of) and np.array_equal(out["obs_id"].cpu().numpy(), oi)
    assert R.same_bits(out["obs_meas"].cpu().numpy(), om)
    assert np.array_equal(out["lm_first"].cpu().numpy(), first)
    assert R.same_bits(out["initial_residuals"].cpu().numpy(), resid)


def test_gate_reference_rule(oracle):
    ref, _, resid, gates = gate_case(oracle)
    assert_gate_case_contents(ref, resid, gates)


@pytest.mark.parametrize("gate_name", ["all", "finite", "none", "first_dropped", "empty"])
def test_gate_factors_filtering_on_the_cpu(oracle, monkeypatch, gate_name):
    """BatchSequence.gate_factors on CPU tensors with the oracle in the residual kernel's place: only the torch
    filtering after the call is under test here (the kernel itself: tests/test_track_emit_gpu.py)."""
    import torch
    from visual_underwater_slam_amd import _lib, sequence

    def call(name, *args):
        assert name == "vus_stereo_initial_residuals"
        assert oracle.lib().vus_stereo_initial_residuals_cpu(*[ctypes.c_void_p(a) for a in args[:6]], int(args[6]),
                                                             ctypes.c_void_p(args[7])) == 0

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    ref, Rt, resid, gates = gate_case(oracle)
    seq = sequence.BatchSequence(disparity_sign=1, device="cpu")
    assert np.array_equal(seq.K.vector6(), R.K6)
    if gate_name == "empty":            # no factor emitted: every landmark stays unseen
        ref = {k: (v[:0] if k.startswith("obs") else v) for k, v in ref.items()}
        ref["lm_first"] = np.full_like(ref["lm_first"], -1)
        resid, g = resid[:0], 60.0
    else:
        g = gates[gate_name]
    factors = {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in ("obs_frame", "obs_id", "obs_meas", "lm_first", "lm_point")}
    out = seq.gate_factors(factors, torch.from_numpy(np.ascontiguousarray(Rt)), g)
    check_gate_output(out, R.gate(resid, g, ref["obs_frame"], ref["obs_id"], ref["obs_meas"], ref["lm_first"]), resid)
    assert R.same_bits(out["lm_point"].numpy(), ref["lm_point"])
