"""The two-view refit of loop closures (LoopClosureParams.refit = "stereo") on the front end's own output, on the closed
track of tests/loop_scene.py with sub-pixel disparities: refine_relative_poses behind relative_poses equals the numpy
statements run on the CPU oracle front end's tables (the front end is bit-exact, so the tables are the same), the
covariance of the measurement follows the whitened rule, and run_sequence takes the second stage through both graph
builders -- and is unchanged, stage for stage and factor for factor, with refit = "left"."""
import dataclasses

import numpy as np
import pytest
import torch

import loop_ref as L
import loop_scene as LS
import pair_bundle_ref as B
import subpixel_ref as S
import subpixel_scene as SS
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

PAIR_A, PAIR_B = [LS.REVISIT[0], 1, LS.FALSE_PAIR[0]], [LS.REVISIT[1], 9, LS.FALSE_PAIR[1]]
REL = 1e-8


@pytest.fixture(scope="module")
def track(gpu):
    from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend
    from visual_underwater_slam_amd.sequence import SEQUENCE_PARAMS, LoopClosureParams
    gt = LS.poses_gt()
    frames = synth.scene_frames(gt, LS.H, LS.W, xp=torch, device="cuda").contiguous()
    fe = StereoOrbFrontend(LS.H, LS.W, max_frames=LS.N_KF, params=ImageProcessorParams(max_features=LS.KP, **SEQUENCE_PARAMS))
    res = fe.process(frames)
    disp, _ = fe.refine_stereo(res, frames, SS.HALF_WIN, SS.SEARCH)
    prm = LoopClosureParams(refit="stereo")
    midx = fe.match_keyframes(res, PAIR_A, PAIR_B, max_distance=LS.MATCH_DISTANCE)
    one = fe.relative_poses(res, PAIR_A, PAIR_B, midx, LS.CAM5, LS.THRESHOLD, LS.N_HYP, synth.SEED, LS.REFINE, disparity=disp)
    kept = {k: getattr(one, k).clone() for k in ("T_ab", "info", "match_idx_out")}
    two = fe.refine_relative_poses(res, one, LS.CAM5, prm.sigma_uv_px, prm.disparity_sigma(True), prm.gate_sigma,
                                   prm.refine_iters, disparity=disp)
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(getattr(one, k), v), k                  # stage one's outputs are inputs here: left alone
    return dict(gt=gt, frames=frames, one=one, two=two, prm=prm)


def test_both_stages_equal_the_reference_on_the_oracle_front_ends_tables(track):
    from oracle import chain, oracle as O
    frames = track["frames"].cpu().numpy()
    fe = chain.frontend(frames, LS.KP, 30, True)
    disp, _ = S.refine(frames.reshape(2 * LS.N_KF, LS.H, LS.W), LS.W, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"],
                       SS.HALF_WIN, SS.SEARCH)
    pa, pb = np.array(PAIR_A, np.int32), np.array(PAIR_B, np.int32)
    fwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pa, 2 * pb, -1, 0, 0, LS.MATCH_DISTANCE)
    bwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pb, 2 * pa, -1, 0, 0, LS.MATCH_DISTANCE)
    t = LS.tables(O.cross_check(fwd, bwd), pa, pb, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"])
    mg = B.Margins()
    r1 = S.stereo_pair_pose_q8(t, disp, LS.THRESHOLD, LS.N_HYP, synth.SEED, LS.REFINE, mg)
    prm = track["prm"]
    r2 = B.stereo_pair_bundle(dict(t, match_idx=r1["match_idx_out"]), r1["T_ab"], r1["info"], prm.sigma_uv_px,
                              prm.disparity_sigma(True), prm.gate_sigma, prm.refine_iters, disp, mg)
    print(f"stage one info {r1['info'].tolist()}, stage two info {r2['info'].tolist()}, {mg}")
    assert mg.safe(), mg                                         # no decision of either reference within rounding of its bound
    one, two = track["one"], track["two"]
    assert np.array_equal(one.info.cpu().numpy(), r1["info"]) and np.array_equal(one.match_idx_out.cpu().numpy(), r1["match_idx_out"])
    assert np.array_equal(two.info.cpu().numpy(), r2["info"]), (two.info.cpu().numpy().tolist(), r2["info"].tolist())
    assert np.array_equal(two.match_idx_out.cpu().numpy(), r2["match_idx_out"])
    from visual_underwater_slam_amd.sequence import loop_closure_measurements
    acc = loop_closure_measurements(two, prm)[0]
    assert acc.tolist() == [True, True, False]                   # the revisit and (1, 9) overlap; (0, 4) share no ground
    assert r2["info"][2, 3] != 0
    for got, k in ((two.T_ab, "T_ab"), (two.S.reshape(-1, 36), "S"), (two.chi2, "chi2"), (two.points, "points")):
        g = got.cpu().numpy()
        err = np.abs(g[acc] - r2[k][acc]).max() / np.abs(r2[k][acc]).max()
        print(f"{k} of the accepted closures: {err:.2e} of its largest entry")
        assert err <= REL, (k, err)
    for c in np.nonzero(acc)[0]:
        truth = LS.relative(track["gt"], PAIR_A[c], PAIR_B[c])
        e1, e2 = L.pose_error(one.T_ab[c].cpu().numpy(), truth)[0], L.pose_error(two.T_ab[c].cpu().numpy(), truth)[0]
        print(f"closure ({PAIR_A[c]}, {PAIR_B[c]}): {1e3 * e1:.1f} mm after the left-image refit, {1e3 * e2:.1f} mm after the two-view refit")


def test_covariance_is_the_whitened_rule_on_the_final_active_points(track):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.sequence import LoopClosureParams, adjoint_map, loop_closure_factors, loop_closure_measurements
    two, prm = track["two"], track["prm"]
    info, S6, chi2 = two.info.cpu().numpy(), two.S.cpu().numpy(), two.chi2.cpu().numpy()
    acc, meas, cov, scale = loop_closure_measurements(two, prm)
    for c in np.nonzero(acc)[0]:
        n = int(info[c, 2])
        s = max(1.0, float(np.sqrt(chi2[c] / (3 * n - 6))))
        assert scale[c] == s and np.allclose(cov[c], s * s * np.linalg.inv(S6[c]), rtol=1e-12, atol=0.0)
        assert np.array_equal(meas[c].flat12(), two.T_ab[c].cpu().numpy())
    # min_inliers counts the final active points (column 2), not the candidates
    n0 = int(info[0, 2])
    assert info[0, 0] > n0
    assert loop_closure_measurements(two, LoopClosureParams(refit="stereo", min_inliers=n0))[0][0]
    assert not loop_closure_measurements(two, LoopClosureParams(refit="stereo", min_inliers=n0 + 1))[0][0]
    # the adjoint, the diagonal sigmas and the robust wrapper are those of the left-image path
    body = gtsam.Pose3(gtsam.Rot3.Rz(0.3), np.array([0.1, -0.05, 0.2]))
    _, mb, cb, _ = loop_closure_measurements(two, prm, body)
    Ad = adjoint_map(body)
    assert np.allclose(cb[0], Ad @ cov[0] @ Ad.T, rtol=1e-12, atol=0.0)
    assert mb[0].equals(body.compose(meas[0]).compose(body.inverse()), 1e-12)
    fs = loop_closure_factors(two, (PAIR_A, PAIR_B), LoopClosureParams(refit="stereo", robust=("Cauchy", 3.0)))
    assert len(fs) == int(acc.sum()) and fs[0].measured().equals(meas[0], 1e-12)
    assert isinstance(fs[0].noiseModel(), gtsam.noiseModel.Robust)
    plain = loop_closure_factors(two, (PAIR_A, PAIR_B), prm)
    assert np.allclose(plain[0].noiseModel().sigmas(), np.sqrt(np.diag(cov[0])), rtol=1e-12, atol=0.0)


def _same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), what
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for q, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (what, q))
    elif dataclasses.is_dataclass(a):
        for f in dataclasses.fields(a):
            _same(getattr(a, f.name), getattr(b, f.name), (what, f.name))
    elif hasattr(a, "kp_keys"):                                   # a FrontendResult: views of two front ends' workspaces
        for k in ("kp_keys", "kp_count", "desc", "stereo_idx", "track_idx"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    else:
        assert a == b, what


def _closures(seq):
    from visual_underwater_slam_amd import gtsam
    return [f for f in seq.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]


def test_run_sequence_left_is_the_default_bit_for_bit_and_stereo_runs_the_second_stage(gpu):
    from visual_underwater_slam_amd import sequence
    from visual_underwater_slam_amd.frontend import PairBundle, PairPoses
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    n = 4
    sc = synth.scene_sequence(n, LS.H, LS.W)
    frames = torch.from_numpy(sc["frames"]).cuda()
    args = (frames, sc["poses_init"], sc["imu"], sc["dvl"])
    near = dict(min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=1)     # neighbours as "closures": they overlap
    poses = lambda r: np.stack([r.atPose3(X(i)).flat12() for i in range(n)])
    for sub in (None, sequence.SubpixelParams()):
        r0, q0, s0 = sequence.run_sequence(*args, disparity_sign=1, subpixel=sub, loop_closure=sequence.LoopClosureParams(**near))
        r1, q1, s1 = sequence.run_sequence(*args, disparity_sign=1, subpixel=sub,
                                           loop_closure=sequence.LoopClosureParams(refit="left", **near))
        _same(s0, s1, "stages")
        assert isinstance(s1["loop_result"], PairPoses) and "loop_stage_one" not in s1
        f0, f1 = _closures(q0), _closures(q1)
        assert len(f0) == len(f1) >= 1 and len(q0.graph._factors) == len(q1.graph._factors)
        for a, b in zip(f0, f1):
            assert list(a.keys()) == list(b.keys()) and np.array_equal(a.measured().flat12(), b.measured().flat12())
            assert np.array_equal(a.noiseModel().sigmas(), b.noiseModel().sigmas())
        assert np.array_equal(poses(r0), poses(r1))
        for bulk in (True, False):
            prm = sequence.LoopClosureParams(refit="stereo", **near)
            r2, q2, s2 = sequence.run_sequence(*args, disparity_sign=1, bulk=bulk, subpixel=sub, loop_closure=prm)
            two, one = s2["loop_result"], s2["loop_stage_one"]
            assert isinstance(two, PairBundle) and isinstance(one, PairPoses)
            if bulk:
                assert set(s2) - set(s0) == {"loop_stage_one"}
            _same(one, s0["loop_result"], "stage one")
            info = two.info.cpu().numpy()
            print(f"subpixel={sub is not None} bulk={bulk}: stage two info {info.tolist()}, accepted {s2['loop_accepted'].tolist()}")
            assert (info[:, 3] == 0).all() and (info[:, 2] <= one.info.cpu().numpy()[:, 3]).all()
            want = sequence.loop_closure_factors(two, s2["loop_pairs"], prm)
            got = _closures(q2)
            assert len(got) == len(want) == int(s2["loop_accepted"].sum()) >= 1
            for a, b in zip(got, want):
                assert list(a.keys()) == list(b.keys()) and np.array_equal(a.measured().flat12(), b.measured().flat12())
                assert np.array_equal(a.noiseModel().sigmas(), b.noiseModel().sigmas())
            assert np.isfinite(poses(r2)).all()
    with pytest.raises(ValueError, match="refit"):
        sequence.LoopClosureParams(refit="right")
