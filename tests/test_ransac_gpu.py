"""vus_two_point_ransac on the GPU against its numpy statement (tests/ransac_ref.py), bit for bit: track_idx_out and
all four info columns, on the adversarial tables, planted scenes at several list sizes, a pair beyond the matches the
kernel keeps in LDS, hypothesis counts below / at / above the block size, batches, and in place."""
import numpy as np
import pytest
import torch

import ransac_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777


def run_gpu(t, threshold_px=R.PLANTED_THRESHOLD, n_hyp=64, seed=20261004, inplace=False):
    from visual_underwater_slam_amd import _lib as L
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    trk = d(t["track_idx"].astype(np.int32))
    keys = d(t["kp_keys"].view(np.int32))
    cnt = d(t["kp_count"].astype(np.int32))
    rot = d(np.asarray(t["rot"], np.float64))
    P, K = t["track_idx"].shape
    out = trk if inplace else torch.full((P, K), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.full((P, 4), SENTINEL, dtype=torch.int32, device="cuda")
    cam = np.ascontiguousarray(t["cam"], np.float64)
    L.call("vus_two_point_ransac", trk.data_ptr(), keys.data_ptr(), cnt.data_ptr(), P + 1, K, t["H"], t["W"], rot.data_ptr(),
           cam.ctypes.data, float(threshold_px), int(n_hyp), int(seed), out.data_ptr(), info.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(trk.cpu().numpy(), t["track_idx"])          # the input is left alone
    return out.cpu().numpy(), info.cpu().numpy()


def check(name, **kw):
    t, (ref_out, ref_info) = R.case(name, **kw)
    out, info = run_gpu(t, **kw)
    assert np.array_equal(info, ref_info), (name, kw, info.tolist(), ref_info.tolist())
    assert not (out == SENTINEL).any()                                     # every slot is written
    bad = np.argwhere(out != ref_out)
    assert len(bad) == 0, (name, kw, len(bad), bad[:5].tolist())
    return t, ref_out, ref_info


@pytest.mark.parametrize("name", list(R.ADVERSARIAL) + [f"planted_kp{k}" for k in R.PLANTED_KP])
def test_kernel_equals_the_reference(gpu, name):
    t, out, info = check(name)
    if name == "planted_kp2000":
        assert info[:, 0].tolist() == [400, 600, 64, 600, 1200] and (info[:, 2] >= 0).all()
        assert (info[:, 1] >= 0.4 * info[:, 0]).all()


def test_pair_beyond_the_lds_resident_matches(gpu):
    """About 4000 matches in 8192 slots: the kernel keeps packed positions in LDS and recomputes the per-match values."""
    t, out, info = check("large")
    assert info[0, 0] > 2000


@pytest.mark.parametrize("n_hyp", [1, 64, 100, 256, 4096])
def test_hypothesis_counts_around_the_block_size(gpu, n_hyp):
    check("planted_kp64", n_hyp=n_hyp)


def test_one_pair_and_a_batch_of_nine(gpu):
    t, _, info = check("batch9", n_hyp=100)
    assert len(info) == 9 and len(set(info[:, 2].tolist())) > 3 and len({tuple(r) for r in t["rot"]}) == 9
    one = {k: (v[:1] if k in ("track_idx", "rot") else v[:4] if k in ("kp_keys", "kp_count") else v) for k, v in t.items()}
    out1, info1 = run_gpu(one, n_hyp=100)
    ref_out, ref_info = R.case("batch9", n_hyp=100)[1]
    assert np.array_equal(out1, ref_out[:1]) and np.array_equal(info1, ref_info[:1])       # n_frames = 2


def test_other_seed_and_threshold(gpu):
    check("planted_kp64", seed=7, threshold_px=1.0)
    check("make_tables", seed=0xFFFFFFFF, threshold_px=40.0, n_hyp=256)


@pytest.mark.parametrize("name", ["make_tables", "planted_kp2000", "large"])
def test_in_place_equals_out_of_place(gpu, name):
    t, (ref_out, ref_info) = R.case(name)
    out, info = run_gpu(t, inplace=True)
    assert np.array_equal(out, ref_out) and np.array_equal(info, ref_info)
