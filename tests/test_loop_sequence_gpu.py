"""Loop closures from the front end's own output on the closed track of tests/loop_scene.py (ten rendered keyframes at
640 x 360, 2 m above the sea floor: 19 px of disparity; the last keyframe revisits the first, turned by 25 degrees):
match_keyframes + relative_poses equal the numpy statement on the same tables, the revisit is accepted and the pair
without common ground is not, the measurement is as accurate as the reference can be, the closure pulls the drifted end of
the track back, and run_sequence is unchanged without the new argument.

The accuracy bound.  On the CPU oracle front end's output for the same frames (oracle/chain.frontend, mutual matches at
Hamming <= 50) the numpy reference finds 281 candidates for the pair (0, 9), keeps 119 of them and returns T_0^-1 T_9
4.77 mm and 1.09e-3 rad off the ground truth; the pair (0, 4) has 101 chance candidates, its best model two inliers, and
ends with status 3 (tools/loop_reference_error.py, profiles/loop_closure.md).  The GPU path is held to twice that:
9.55 mm and 2.18e-3 rad."""
import numpy as np
import pytest
import torch

import loop_ref as L
import loop_scene as S
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

REF_ERROR_M, REF_ERROR_RAD = 4.77e-3, 1.09e-3          # measured on the CPU, see the docstring
PAIR_A, PAIR_B = [S.REVISIT[0], S.FALSE_PAIR[0]], [S.REVISIT[1], S.FALSE_PAIR[1]]


@pytest.fixture(scope="module")
def track(gpu):
    gt = S.poses_gt()
    frames = synth.scene_frames(gt, S.H, S.W, xp=torch, device="cuda")
    return dict(gt=gt, init=S.poses_drifted(gt), frames=frames.contiguous())


@pytest.fixture(scope="module")
def front(track):
    from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend
    from visual_underwater_slam_amd.sequence import SEQUENCE_PARAMS
    fe = StereoOrbFrontend(S.H, S.W, max_frames=S.N_KF, params=ImageProcessorParams(max_features=S.KP, **SEQUENCE_PARAMS))
    res = fe.process(track["frames"])
    midx = fe.match_keyframes(res, PAIR_A, PAIR_B, max_distance=S.MATCH_DISTANCE)
    poses = fe.relative_poses(res, PAIR_A, PAIR_B, midx, S.CAM5, S.THRESHOLD, S.N_HYP, synth.SEED, S.REFINE)
    torch.cuda.synchronize()
    return fe, res, midx, poses


def test_gpu_equals_the_reference_on_the_front_ends_tables(front):
    fe, res, midx, poses = front
    t = S.tables(midx.cpu().numpy(), PAIR_A, PAIR_B, res.stereo_idx.cpu().numpy(), res.kp_keys.cpu().numpy(),
                 res.kp_count.cpu().numpy())
    mg = L.Margins()
    ref = L.stereo_pair_pose(t, S.THRESHOLD, S.N_HYP, synth.SEED, S.REFINE, mg)
    print(f"front-end tables: info {ref['info'].tolist()}, {mg}")
    assert mg.safe(), mg                                     # no decision of the reference within rounding of its bound
    assert np.array_equal(poses.info.cpu().numpy(), ref["info"]), (poses.info.cpu().numpy().tolist(), ref["info"].tolist())
    assert np.array_equal(poses.match_idx_out.cpu().numpy(), ref["match_idx_out"])
    for got, k in ((poses.T_ab, "T_ab"), (poses.JtJ.reshape(-1, 36), "JtJ"), (poses.rss, "rss")):
        err = np.abs(got.cpu().numpy() - ref[k]).max() / np.abs(ref[k]).max()
        print(f"{k}: {err:.2e} of its largest entry")
        assert err <= 1e-8, (k, err)
    # the mutual filter did its work: a match of a -> b is also the match of b -> a
    back = fe.match_keyframes(res, PAIR_B, PAIR_A, max_distance=S.MATCH_DISTANCE).cpu().numpy()
    m = midx.cpu().numpy()
    for c in range(2):
        src = np.nonzero(m[c] >= 0)[0]
        assert len(src) > 50 and np.array_equal(back[c, m[c, src]], src)
    loose = fe.match_keyframes(res, PAIR_A, PAIR_B, max_distance=S.MATCH_DISTANCE, cross_check=False).cpu().numpy()
    assert ((loose >= 0).sum(1) > (m >= 0).sum(1)).all() and np.array_equal(loose[m >= 0], m[m >= 0])


def test_revisit_is_accepted_and_accurate_and_the_false_candidate_is_not(front, track):
    from visual_underwater_slam_amd.sequence import LoopClosureParams, loop_closure_factors, loop_closure_measurements
    fe, res, midx, poses = front
    prm = LoopClosureParams()
    acc, meas, cov, scale = loop_closure_measurements(poses, prm)
    info = poses.info.cpu().numpy()
    et, er = L.pose_error(poses.T_ab[0].cpu().numpy(), S.relative(track["gt"], *S.REVISIT))
    print(f"revisit {S.REVISIT}: info {info[0].tolist()}, error {1e3 * et:.2f} mm {er:.2e} rad, s = {scale[0]:.3f} px, sigmas "
          f"{np.sqrt(np.diag(cov[0])).tolist()}; no overlap {S.FALSE_PAIR}: info {info[1].tolist()}")
    assert acc.tolist() == [True, False]
    assert info[0, 4] == 0 and info[0, 3] >= prm.min_inliers and info[0, 0] >= 18 * 3
    assert not (info[1, 4] == 0 and info[1, 3] >= prm.min_inliers)
    assert et <= 2 * REF_ERROR_M and er <= 2 * REF_ERROR_RAD, (et, er)
    fs = loop_closure_factors(poses, (PAIR_A, PAIR_B), prm)
    assert len(fs) == 1 and fs[0].measured().equals(meas[0], 1e-12)


def _last_position_error(track, fe, res, closures):
    """LM on the stereo factors of the track, a prior on X(0) and `closures`, from the drifted poses."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import L as LM, X
    from visual_underwater_slam_amd.sequence import GATE_PX, BatchSequence
    seq = BatchSequence(disparity_sign=1)
    ids, feats, n_ids = fe.feature_tracks(res)
    Rt = torch.from_numpy(track["init"]).cuda()
    fac = seq.gate_factors(fe.stereo_factors(ids, feats, n_ids, Rt, seq.cam_array(), first_frame=0), Rt, GATE_PX)
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(track["init"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(np.array([1e-3] * 3 + [1e-3] * 3))))
    kx = fac["obs_frame"].cpu().numpy().astype(np.int64) + X(0)
    kl = fac["obs_id"].cpu().numpy().astype(np.int64) + LM(0)
    graph.push_back(gtsam.StereoFactorBlock(fac["obs_meas"].cpu().numpy(), seq.landmark_noise, kx, kl, seq.K))
    for k in range(S.N_KF):
        values.insert(X(k), gtsam.Pose3.from_flat12(track["init"][k]))
    seen = np.nonzero(fac["lm_first"].cpu().numpy() >= 0)[0]
    values.insert_point3_block(seen.astype(np.int64) + LM(0), fac["lm_point"].cpu().numpy()[seen])
    for f in closures:
        graph.push_back(f)
    out = gtsam.LevenbergMarquardtOptimizer(graph, values).optimize()
    last = S.N_KF - 1
    return float(np.linalg.norm(out.atPose3(X(last)).translation() - track["gt"][last, 9:])), len(kx)


def test_closure_pulls_the_end_of_the_track_back(front, track):
    from visual_underwater_slam_amd.sequence import LoopClosureParams, loop_closure_factors
    fe, res, midx, poses = front
    closures = loop_closure_factors(poses, (PAIR_A, PAIR_B), LoopClosureParams())
    assert len(closures) == 1
    start = float(np.linalg.norm(track["init"][-1, 9:] - track["gt"][-1, 9:]))
    without, n_fac = _last_position_error(track, fe, res, [])
    with_closure, _ = _last_position_error(track, fe, res, closures)
    print(f"last keyframe's position error: {1e3 * start:.1f} mm at the start, {1e3 * without:.2f} mm after LM on {n_fac} "
          f"stereo factors, {1e3 * with_closure:.2f} mm with the closure X(0)-X(9)")
    assert with_closure < without, (with_closure, without)


def test_run_sequence_is_unchanged_without_loop_closure_and_gains_stages_with_it(gpu):
    from visual_underwater_slam_amd import gtsam, sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    n = 4
    sc = synth.scene_sequence(n, S.H, S.W)
    frames = torch.from_numpy(sc["frames"]).cuda()
    args = (frames, sc["poses_init"], sc["imu"], sc["dvl"])
    r0, _, s0 = sequence.run_sequence(*args, disparity_sign=1)
    r1, _, s1 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=None)
    assert set(s0) == set(s1) and not any(k.startswith("loop") for k in s0)
    p0 = np.stack([r0.atPose3(X(i)).flat12() for i in range(n)])
    assert np.array_equal(p0, np.stack([r1.atPose3(X(i)).flat12() for i in range(n)]))
    # neighbours as "closures" (min_gap = 1): they overlap, so the path is exercised end to end on both graph builders
    prm = sequence.LoopClosureParams(min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=1)
    counts = []
    for bulk in (True, False):
        r2, seq2, s2 = sequence.run_sequence(*args, disparity_sign=1, bulk=bulk, loop_closure=prm)
        assert {"loop_pairs", "loop_result", "loop_accepted"} <= set(s2)
        if bulk:
            assert set(s2) - set(s0) == {"loop_pairs", "loop_result", "loop_accepted"}
        pa, pb = s2["loop_pairs"]
        assert pa.tolist() == [0, 1, 2] and pb.tolist() == [1, 2, 3]
        btw = [f for f in seq2.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
        assert len(btw) == int(s2["loop_accepted"].sum()) >= 1
        counts.append(len(btw))
        info = s2["loop_result"].info.cpu().numpy()
        print(f"bulk={bulk}: info {info.tolist()}, accepted {s2['loop_accepted'].tolist()}")
        for f in btw:      # printed, not asserted: at 4 m the disparity is 9.6 px, below what the accuracy tests use
            a, b = (int(k - X(0)) for k in f.keys())
            want = gtsam.Pose3.from_flat12(sc["poses_gt"][a]).between(gtsam.Pose3.from_flat12(sc["poses_gt"][b]))
            print(f"  X({a})-X({b}): {1e3 * np.linalg.norm(f.measured().translation() - want.translation()):.1f} mm off")
        p2 = np.stack([r2.atPose3(X(i)).flat12() for i in range(n)])
        assert np.isfinite(p2).all()
    assert counts[0] == counts[1]
    # no candidate at all: the keys are there, nothing is launched
    _, seq3, s3 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=sequence.LoopClosureParams(min_gap=n))
    assert s3["loop_result"] is None and len(s3["loop_pairs"][0]) == 0 and len(s3["loop_accepted"]) == 0
    assert not [f for f in seq3.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
