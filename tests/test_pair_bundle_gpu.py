"""vus_stereo_pair_bundle on the GPU against its numpy statement (tests/pair_bundle_ref.py) on fixtures the reference
certifies as margin-safe: info (all six columns) and match_idx_out EQUAL; T_ab, S, chi2 and points within 1e-8 of the
largest entry of each array -- the bound tests/test_loop_gpu.py holds the same kind of sums to: only the summation order,
the form of the back-substitution and the libm calls of the retraction differ.  Outputs are prefilled with a sentinel:
every slot must be written."""
import numpy as np
import pytest
import torch

import loop_ref as R
import pair_bundle_ref as B

pytestmark = pytest.mark.gpu

SENTINEL = -777
FSENT = -7.77e77
REL = 1e-8
FLOATS = ("T_ab", "S", "chi2", "points")


def run_gpu(t, T_in, info_in, sigma_uv_px=B.SIGMA_UV, sigma_disp_px=B.SIGMA_D, gate=B.GATE, iters=B.ITERS, disp_q8=None,
            inplace=False):
    from visual_underwater_slam_amd import _lib as L
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mt = d(t["match_idx"].astype(np.int32))
    pa, pb = d(t["pair_a"].astype(np.int32)), d(t["pair_b"].astype(np.int32))
    st = d(t["stereo_idx"].astype(np.int32))
    keys = d(t["kp_keys"].view(np.int32))
    cnt = d(t["kp_count"].astype(np.int32))
    Tin, iin = d(np.asarray(T_in, np.float64)), d(np.asarray(info_in, np.int32))
    q8 = None if disp_q8 is None else d(np.asarray(disp_q8, np.int32))
    P, K = t["match_idx"].shape
    F = len(t["stereo_idx"])
    out = mt if inplace else torch.full((P, K), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.full((P, 6), SENTINEL, dtype=torch.int32, device="cuda")
    T = torch.full((P, 12), FSENT, dtype=torch.float64, device="cuda")
    S = torch.full((P, 36), FSENT, dtype=torch.float64, device="cuda")
    chi2 = torch.full((P,), FSENT, dtype=torch.float64, device="cuda")
    pts = torch.full((P, K, 3), FSENT, dtype=torch.float64, device="cuda")
    cam = np.ascontiguousarray(t["cam"], np.float64)
    L.call("vus_stereo_pair_bundle", mt.data_ptr(), pa.data_ptr(), pb.data_ptr(), st.data_ptr(), keys.data_ptr(), cnt.data_ptr(),
           F, P, K, t["H"], t["W"], cam.ctypes.data, None if q8 is None else q8.data_ptr(), Tin.data_ptr(), iin.data_ptr(),
           float(sigma_uv_px), float(sigma_disp_px), float(gate), int(iters), T.data_ptr(), S.data_ptr(), chi2.data_ptr(),
           pts.data_ptr(), out.data_ptr(), info.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(mt.cpu().numpy(), t["match_idx"])           # the input is left alone
    assert np.array_equal(Tin.cpu().numpy(), np.asarray(T_in, np.float64))     # T_in and info_in are unchanged afterwards
    assert np.array_equal(iin.cpu().numpy(), np.asarray(info_in, np.int32))
    for a, b in ((st, t["stereo_idx"]), (pa, t["pair_a"]), (cnt, t["kp_count"])):
        assert np.array_equal(a.cpu().numpy(), b)
    return dict(T_ab=T.cpu().numpy(), S=S.cpu().numpy(), chi2=chi2.cpu().numpy(), points=pts.cpu().numpy(),
                match_idx_out=out.cpu().numpy(), info=info.cpu().numpy())


def written(got, what):
    assert not (got["match_idx_out"] == SENTINEL).any() and not (got["info"] == SENTINEL).any(), what
    for k in FLOATS:
        assert np.isfinite(got[k]).all() and not (got[k] == FSENT).any(), (what, k)
    s = got["S"].reshape(-1, 6, 6)
    assert np.array_equal(s, s.transpose(0, 2, 1))


def compare(got, ref, what):
    assert np.array_equal(got["info"], ref["info"]), (what, got["info"].tolist(), ref["info"].tolist())
    written(got, what)
    bad = np.argwhere(got["match_idx_out"] != ref["match_idx_out"])
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())
    for k in FLOATS:
        scale = max(np.abs(ref[k]).max(), 1e-300)
        err = np.abs(got[k] - ref[k]).max() / scale
        print(f"{what}: {k} differs by {err:.2e} of its largest entry {scale:.3g}")
        assert err <= REL, (what, k, err)
    assert np.array_equal(got["points"].any(-1), got["match_idx_out"] >= 0)       # a point for every active slot and no other


def check(name, **kw):
    t, T_in, info_in, ref = B.case(name, **kw)
    got = run_gpu(t, T_in, info_in, **{k: v for k, v in kw.items() if k != "n_hyp"})      # n_hyp is stage one's
    compare(got, ref, (name, kw))
    return t, T_in, info_in, ref, got


@pytest.mark.parametrize("name", ["no_disparity", "identical", "pairing", "bad_tables"] + [f"planted_kp{k}" for k in R.PLANTED_KP])
def test_kernel_equals_the_reference_behind_stage_one(gpu, name):
    """Stage one's outputs (the reference's) on its adversarial tables -- refused and shared frames, counts and indices out
    of range, identical frames -- and on planted scenes at max_kp = 1, 64, 65, 257, 2000 and 4096."""
    t, T_in, info_in, ref, got = check(name)
    if name.startswith("planted_kp") and name not in ("planted_kp1",):
        assert (ref["info"][:, 3] == 0).any() and ref["info"][:, 2].max() >= 30
    if name == "identical":
        assert np.abs(got["T_ab"] - R.IDENTITY12).max() <= 1e-9


@pytest.mark.parametrize("name", ["few", "gated", "passed"])
def test_few_candidates_a_failed_solve_and_a_passed_through_pair(gpu, name):
    """n = 0..4 candidates (status 1 below three; three candidates of which the gate keeps two: status 3 by count); a start
    so far off that no point passes the gate, beside a live pair; a pair stage one refused beside a live one."""
    t, T_in, info_in, ref = B.explicit_case(name)
    got = run_gpu(t, T_in, info_in)
    compare(got, ref, name)
    if name == "passed":
        assert got["info"][0].tolist() == [0, 0, 0, 4, 0, 0] and np.array_equal(got["T_ab"][0], T_in[0])
        assert got["info"][1, 3] == 0 and got["info"][1, 2] >= 30


def test_every_slot_a_candidate_at_the_lds_maximum(gpu):
    """max_kp = 4096 with stage one's INPUT table: all 4096 slots of pair 0 are candidates, the 1496 wrong matches among
    them are the gate's business."""
    t, T_in, info_in = B.stage_one("planted_kp4096")
    raw = dict(t, match_idx=R.tables("planted_kp4096")["match_idx"])
    ref = B.certify("raw4096", raw, T_in, info_in)
    assert ref["info"][0, 0] == 4096 and 1500 < ref["info"][0, 2] < 2700
    compare(run_gpu(raw, T_in, info_in), ref, "raw4096")


@pytest.mark.parametrize("name", ["collinear", "duplicate"])
def test_singular_point_sets_end_defined(gpu, name):
    """Points on one line, and twelve copies of one point: S is singular, its later pivots are rounding errors of either
    sign, so neither the reference nor the kernel is held to a status; whichever way they fall, every slot is written,
    the candidates are counted alike, and a pair that ends with status 3 reports nothing.

    Measured: the reference ends both with status 3 in round 0, at pivots 1.8e-11 (collinear) and 6.6e-16 (duplicate) of
    their diagonal entries -- far below the 1e-9 a certified fixture needs.  The MI355X kernel ends the duplicate set with
    status 3 as well, info (12, 12, 0, 3, 0, 0), and the collinear set with status 0 after ten rounds, info
    (40, 40, 40, 0, 10, 0): there the same pivot rounded to the positive side."""
    t, T_in, info_in = B.degenerate_tables(name)
    ref = B.stereo_pair_bundle(t, T_in, info_in, B.SIGMA_UV, B.SIGMA_D, B.GATE, B.ITERS)
    got = run_gpu(t, T_in, info_in)
    written(got, name)
    print(f"{name}: kernel info {got['info'].tolist()}, reference info {ref['info'].tolist()}")
    assert got["info"][0, 0] == ref["info"][0, 0] and got["info"][0, 1] == ref["info"][0, 1]
    assert got["info"][0, 3] in (0, 3)
    if got["info"][0, 3] == 3:
        assert not got["S"].any() and not got["chi2"].any() and not got["points"].any() and (got["match_idx_out"] == -1).all()
        assert got["info"][0, 2] == 0


@pytest.mark.parametrize("iters", [0, 10])
def test_without_and_with_rounds(gpu, iters):
    t, T_in, info_in, ref, got = check("planted_kp2000", n_hyp=256, iters=iters)
    live = ref["info"][:, 3] == 0
    assert live.all() and (ref["info"][:, 4] == iters).all()
    if iters == 0:
        assert np.array_equal(ref["info"][:, 1], ref["info"][:, 2]) and np.array_equal(got["T_ab"], T_in)


def test_one_pair_and_a_batch_of_nine_sharing_frames(gpu):
    """Nine pairs on five frames, every frame in three or four pairs, nine poses and sizes: indexing T_in, info_in, the
    tables or an output by the wrong pair or frame shows."""
    t, T_in, info_in, ref, got = check("shared9")
    assert len(ref["info"]) == 9 and (ref["info"][:, 3] == 0).sum() >= 8 and len(set(ref["info"][:, 0].tolist())) > 5
    one = dict(t, match_idx=t["match_idx"][:1], pair_a=t["pair_a"][:1], pair_b=t["pair_b"][:1])
    got1 = run_gpu(one, T_in[:1], info_in[:1])
    for k in got1:
        assert np.array_equal(got1[k], got[k][:1]), k                      # pair 0 alone: the same bits
    check("batch9", n_hyp=100)


def test_other_sigmas_and_gate(gpu):
    check("planted_kp257", sigma_uv_px=1.0, sigma_disp_px=0.12, gate=3.0)
    check("bad_tables", sigma_uv_px=0.3, sigma_disp_px=1.0, gate=10.0, n_hyp=256)


@pytest.mark.parametrize("name", ["planted_kp257", "bad_tables"])
def test_q8_of_the_integer_disparities_gives_the_bits_of_the_null_call(gpu, name):
    import subpixel_ref as SP
    t, T_in, info_in, ref = B.case(name)
    q8 = SP.integer_disparity_q8(t["stereo_idx"], t["kp_keys"], t["kp_count"], t["W"])
    plain, withq = run_gpu(t, T_in, info_in), run_gpu(t, T_in, info_in, disp_q8=q8)
    compare(plain, ref, name)
    for k in plain:
        assert np.array_equal(plain[k], withq[k]), k


def test_refined_disparities_equal_the_reference(gpu):
    """Q8 disparities that are not multiples of 256: the integer ones moved by up to +-0.4 px."""
    t, T_in, info_in = B.stage_one("planted_kp257")
    import subpixel_ref as SP
    q8 = SP.integer_disparity_q8(t["stereo_idx"], t["kp_keys"], t["kp_count"], t["W"])
    rng = np.random.default_rng(81)
    q8 = np.where(q8 > 0, q8 + rng.integers(-102, 103, q8.shape), 0).astype(np.int32)
    ref = B.certify("planted_kp257_q8", t, T_in, info_in, disp_q8=q8)
    assert (ref["info"][:, 3] == 0).all()
    compare(run_gpu(t, T_in, info_in, disp_q8=q8), ref, "planted_kp257_q8")


@pytest.mark.parametrize("name", ["bad_tables", "pairing", "planted_kp2000", "planted_kp4096"])
def test_in_place_equals_out_of_place_and_a_second_run_is_bit_identical(gpu, name):
    t, T_in, info_in, ref = B.case(name)
    first, again, inplace = run_gpu(t, T_in, info_in), run_gpu(t, T_in, info_in), run_gpu(t, T_in, info_in, inplace=True)
    compare(first, ref, name)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], inplace[k]), k
