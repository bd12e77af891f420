"""vus_stereo_pair_pose on the GPU against its numpy statement (tests/loop_ref.py) on fixtures the reference certifies as
margin-safe: info (all six columns) and match_idx_out EQUAL; T_ab, JtJ and rss within 1e-8 of the largest entry of each
array -- only the summation order and the libm calls of the retraction differ, cond(H) n eps <~ 1e4 * 4096 * 1.1e-16 =
5e-9.  Outputs are prefilled with a sentinel: every slot must be written."""
import numpy as np
import pytest
import torch

import loop_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777
FSENT = -7.77e77
REL = 1e-8


def run_gpu(t, threshold_px=R.THRESHOLD, n_hyp=R.N_HYP, seed=R.SEED, refine_iters=R.REFINE, inplace=False):
    from visual_underwater_slam_amd import _lib as L
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mt = d(t["match_idx"].astype(np.int32))
    pa, pb = d(t["pair_a"].astype(np.int32)), d(t["pair_b"].astype(np.int32))
    st = d(t["stereo_idx"].astype(np.int32))
    keys = d(t["kp_keys"].view(np.int32))
    cnt = d(t["kp_count"].astype(np.int32))
    P, K = t["match_idx"].shape
    F = len(t["stereo_idx"])
    out = mt if inplace else torch.full((P, K), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.full((P, 6), SENTINEL, dtype=torch.int32, device="cuda")
    T = torch.full((P, 12), FSENT, dtype=torch.float64, device="cuda")
    JtJ = torch.full((P, 36), FSENT, dtype=torch.float64, device="cuda")
    rss = torch.full((P,), FSENT, dtype=torch.float64, device="cuda")
    cam = np.ascontiguousarray(t["cam"], np.float64)
    L.call("vus_stereo_pair_pose", mt.data_ptr(), pa.data_ptr(), pb.data_ptr(), st.data_ptr(), keys.data_ptr(), cnt.data_ptr(),
           F, P, K, t["H"], t["W"], cam.ctypes.data, float(threshold_px), int(n_hyp), int(seed), int(refine_iters),
           T.data_ptr(), JtJ.data_ptr(), rss.data_ptr(), out.data_ptr(), info.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(mt.cpu().numpy(), t["match_idx"])           # the input is left alone
    for a, b in ((st, t["stereo_idx"]), (pa, t["pair_a"]), (cnt, t["kp_count"])):
        assert np.array_equal(a.cpu().numpy(), b)
    return dict(T_ab=T.cpu().numpy(), JtJ=JtJ.cpu().numpy(), rss=rss.cpu().numpy(), match_idx_out=out.cpu().numpy(),
                info=info.cpu().numpy())


def compare(got, ref, what):
    assert np.array_equal(got["info"], ref["info"]), (what, got["info"].tolist(), ref["info"].tolist())
    assert not (got["match_idx_out"] == SENTINEL).any()                    # every slot is written
    bad = np.argwhere(got["match_idx_out"] != ref["match_idx_out"])
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())
    for k in ("T_ab", "JtJ", "rss"):
        assert np.isfinite(got[k]).all() and not (got[k] == FSENT).any(), (what, k)
        scale = max(np.abs(ref[k]).max(), 1e-300)
        err = np.abs(got[k] - ref[k]).max() / scale
        print(f"{what}: {k} differs by {err:.2e} of its largest entry {scale:.3g}")
        assert err <= REL, (what, k, err)
    jt = got["JtJ"].reshape(-1, 6, 6)
    assert np.array_equal(jt, jt.transpose(0, 2, 1))


def check(name, **kw):
    t, ref = R.case(name, **kw)
    got = run_gpu(t, **kw)
    compare(got, ref, (name, kw))
    return t, ref, got


@pytest.mark.parametrize("name", list(R.ADVERSARIAL) + [f"planted_kp{k}" for k in R.PLANTED_KP])
def test_kernel_equals_the_reference(gpu, name):
    """The adversarial tables (n = 0..4, collinear, no disparity, identical frames, refused and shared frames, counts and
    indices out of range) and planted scenes at max_kp = 1, 64, 65, 257, 2000 and 4096 (the LDS maximum)."""
    t, ref, got = check(name)
    if name == "planted_kp4096":
        assert ref["info"][0, 0] == 4096
    if name == "identical":
        assert np.abs(got["T_ab"] - R.IDENTITY12).max() <= 1e-9


@pytest.mark.parametrize("n_hyp", [1, 64, 100, 256, 4096])
def test_hypothesis_counts_around_the_block_size(gpu, n_hyp):
    check("planted_kp257", n_hyp=n_hyp)


@pytest.mark.parametrize("refine_iters", [0, 10])
def test_without_and_with_refit(gpu, refine_iters):
    t, ref, got = check("planted_kp2000", n_hyp=256, refine_iters=refine_iters)
    assert (ref["info"][:, 5] == refine_iters).all()
    if refine_iters == 0:
        assert np.array_equal(ref["info"][:, 2], ref["info"][:, 3])


def test_one_pair_and_a_batch_of_nine(gpu):
    t, ref, got = check("batch9", n_hyp=100)
    assert len(ref["info"]) == 9 and len(set(ref["info"][:, 1].tolist())) > 3
    one = dict(t, match_idx=t["match_idx"][:1], pair_a=t["pair_a"][:1], pair_b=t["pair_b"][:1])
    got1 = run_gpu(one, n_hyp=100)
    for k in got1:
        assert np.array_equal(got1[k], got[k][:1]), k                      # pair 0 alone: the same bits


def test_other_seed_and_threshold(gpu):
    check("planted_kp257", seed=7, threshold_px=1.0)
    check("bad_tables", seed=0xFFFFFFFF, threshold_px=6.0, n_hyp=256)


@pytest.mark.parametrize("name", ["bad_tables", "pairing", "planted_kp2000", "planted_kp4096"])
def test_in_place_equals_out_of_place_and_a_second_run_is_bit_identical(gpu, name):
    t, ref = R.case(name)
    first, again, inplace = run_gpu(t), run_gpu(t), run_gpu(t, inplace=True)
    compare(first, ref, name)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], inplace[k]), k
