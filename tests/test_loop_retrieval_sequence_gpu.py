"""Loop-closure candidates by appearance on the closed track of tests/loop_scene.py, from the GPU front end's own output:
keyframe_similarity equals the numpy statement on the same descriptors and ranks the revisit first; with an odometry that
has drifted 1.8 m at the last keyframe pose proximity no longer proposes the revisit, appearance does, and the pair is
measured and accepted as accurately as the reference can; run_sequence is unchanged in "pose" mode and gains exactly
"loop_similarity" otherwise.

The accuracy bound.  The RANSAC samples of a pair depend on its position in the pair list, so the figure is measured for
THIS list: on the CPU oracle front end's output (oracle/chain.frontend) the numpy statements -- retrieval_ref,
appearance_candidates with the default parameters, the oracle matcher (mutual, Hamming <= 50) and loop_ref -- propose
(1,6) (2,7) (1,7) (1,8) (0,8) (0,9) (1,9), accept all seven, and return T_0^-1 T_9 (281 candidates, 119 final inliers)
4.77 mm and 1.09e-3 rad off the ground truth (tools/loop_retrieval_reference.py, profiles/loop_retrieval.md).  The GPU
path is held to twice that: 9.55 mm and 2.18e-3 rad."""
import numpy as np
import pytest
import torch

import loop_ref as L
import loop_scene as S
import retrieval_scene as RS
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

REF_ERROR_M, REF_ERROR_RAD = 4.7746e-3, 1.0902e-3      # measured on the CPU, see the docstring
REF_PAIRS = [(1, 6), (2, 7), (1, 7), (1, 8), (0, 8), (0, 9), (1, 9)]
# The footprint of a keyframe is 2.1 m x 1.2 m on the sea floor; turned by up to 25 degrees it reaches 1.2 m along the track.
# Camera centres 2.3 m apart or more share no ground: (0, 4), (0, 5), (4, 9) and (5, 9) on this track.
NO_GROUND_M = 2.3


@pytest.fixture(scope="module")
def track(gpu):
    gt = S.poses_gt()
    frames = synth.scene_frames(gt, S.H, S.W, xp=torch, device="cuda")
    return dict(gt=gt, far=RS.poses_far_drifted(gt), frames=frames.contiguous())


@pytest.fixture(scope="module")
def front(track):
    from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend
    from visual_underwater_slam_amd.sequence import SEQUENCE_PARAMS
    fe = StereoOrbFrontend(S.H, S.W, max_frames=S.N_KF, params=ImageProcessorParams(max_features=S.KP, **SEQUENCE_PARAMS))
    res = fe.process(track["frames"])
    torch.cuda.synchronize()
    return fe, res


def _pairs(p):
    return list(zip(p[0].tolist(), p[1].tolist()))


def test_similarity_equals_the_reference_and_ranks_the_revisit(front):
    from visual_underwater_slam_amd.sequence import LoopClosureParams, appearance_candidates
    fe, res = front
    prm = LoopClosureParams(candidates="appearance")
    desc, kc = res.desc.cpu().numpy().view(np.uint64), res.kp_count.cpu().numpy()
    for min_gap in (0, prm.min_gap):
        Sg = fe.keyframe_similarity(res, prm.appearance_top, prm.appearance_max_distance, min_gap)
        assert Sg.dtype == torch.int32 and Sg.is_cuda and tuple(Sg.shape) == (S.N_KF, S.N_KF)
        Sm = Sg.cpu().numpy()
        print(Sm)
        assert np.array_equal(Sm, RS.similarity_ref(desc, kc, S.N_KF, prm.appearance_top, prm.appearance_max_distance, min_gap))
        RS.check_ranking(Sm, prm, appearance_candidates(Sg, prm))
    # other settings of the score: every keypoint, the matcher's bound
    Sw = fe.keyframe_similarity(res, top=S.KP, max_distance=50).cpu().numpy()
    assert np.array_equal(Sw, RS.similarity_ref(desc, kc, S.N_KF, S.KP, 50))


def test_appearance_proposes_the_revisit_that_pose_proximity_misses(front, track):
    from visual_underwater_slam_amd.sequence import (LoopClosureParams, appearance_candidates, loop_candidates,
                                                     loop_closure_factors, loop_closure_measurements)
    fe, res = front
    gt, far = track["gt"], track["far"]
    assert np.linalg.norm(far[-1, 9:] - gt[-1, 9:]) > 1.8 > LoopClosureParams().radius_m
    assert S.REVISIT not in _pairs(loop_candidates(far, LoopClosureParams()))                      # "pose": never proposed
    prm = LoopClosureParams(candidates="appearance")
    Sg = fe.keyframe_similarity(res, prm.appearance_top, prm.appearance_max_distance, prm.min_gap)
    pa, pb = appearance_candidates(Sg, prm)
    pairs = _pairs((pa, pb))
    print(f"proposed: {pairs}")
    assert pairs == REF_PAIRS                                                                      # the list the bound was measured on
    midx = fe.match_keyframes(res, pa, pb, max_distance=prm.match_max_distance)
    poses = fe.relative_poses(res, pa, pb, midx, S.CAM5, prm.threshold_px, prm.n_hyp, prm.seed, prm.refine_iters)
    acc, meas, cov, scale = loop_closure_measurements(poses, prm)
    info = poses.info.cpu().numpy()
    T = poses.T_ab.cpu().numpy()
    for c, (a, b) in enumerate(pairs):
        et, er = L.pose_error(T[c], S.relative(gt, a, b))
        apart = float(np.linalg.norm(gt[a, 9:] - gt[b, 9:]))
        print(f"({a}, {b}): score {int(Sg[b, a])}, centres {apart:.2f} m apart, info {info[c].tolist()}, accepted {bool(acc[c])}, "
              f"error {1e3 * et:.2f} mm {er:.2e} rad")
        assert apart < NO_GROUND_M or not acc[c], (a, b)     # nothing without common ground is accepted
    c = pairs.index(S.REVISIT)
    assert acc[c] and info[c, 4] == 0 and info[c, 3] >= prm.min_inliers
    et, er = L.pose_error(T[c], S.relative(gt, *S.REVISIT))
    assert et <= 2 * REF_ERROR_M and er <= 2 * REF_ERROR_RAD, (et, er)
    fs = loop_closure_factors(poses, (pa, pb), prm)
    assert len(fs) == int(acc.sum()) and any(f.measured().equals(meas[c], 1e-12) for f in fs)


def test_run_sequence_is_unchanged_in_pose_mode_and_gains_loop_similarity_otherwise(gpu):
    from visual_underwater_slam_amd import gtsam, sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    n = 4
    sc = synth.scene_sequence(n, S.H, S.W)
    frames = torch.from_numpy(sc["frames"]).cuda()
    args = (frames, sc["poses_init"], sc["imu"], sc["dvl"])
    flat = lambda r: np.stack([r.atPose3(X(i)).flat12() for i in range(n)])
    loop_keys = {"loop_pairs", "loop_result", "loop_accepted"}
    r0, _, s0 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=None)
    assert not any(k.startswith("loop") for k in s0)
    # parameters left at their defaults: pose mode, no keyframe five back on this short track -- the same poses, bit for bit
    r1, _, s1 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=sequence.LoopClosureParams())
    assert set(s1) - set(s0) == loop_keys and set(s0) <= set(s1)
    assert np.array_equal(flat(r0), flat(r1))
    # neighbours as "closures" (min_gap = 1), by pose and by appearance
    near = dict(min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=1)
    r2, _, s2 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=sequence.LoopClosureParams(**near))
    assert set(s2) == set(s1) and _pairs(s2["loop_pairs"]) == [(0, 1), (1, 2), (2, 3)]
    prm = sequence.LoopClosureParams(candidates="appearance", **near)
    r3, seq3, s3 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=prm)
    assert set(s3) - set(s2) == {"loop_similarity"} and set(s2) <= set(s3)
    Sg = s3["loop_similarity"]
    assert Sg.dtype == torch.int32 and Sg.is_cuda and tuple(Sg.shape) == (n, n)
    res = s3["frontend"]
    want = RS.similarity_ref(res.desc.cpu().numpy().view(np.uint64), res.kp_count.cpu().numpy(), n, prm.appearance_top,
                             prm.appearance_max_distance, prm.min_gap)
    print(Sg.cpu().numpy())
    assert np.array_equal(Sg.cpu().numpy(), want)
    assert _pairs(s3["loop_pairs"]) == _pairs(sequence.appearance_candidates(want, prm))
    assert _pairs(s3["loop_pairs"]) == [(0, 1), (1, 2), (1, 3)]            # the CPU oracle front end's answer: S[3] = 90, 96, 85
    btw = [f for f in seq3.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
    assert len(btw) == int(s3["loop_accepted"].sum()) >= 1
    assert np.isfinite(flat(r3)).all()
    # both: the union, ordered by (b, a)
    both = sequence.LoopClosureParams(candidates="both", min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=2)
    _, _, s4 = sequence.run_sequence(*args, disparity_sign=1, loop_closure=both)
    assert set(s4) == set(s3)
    got = _pairs(s4["loop_pairs"])
    one = dict(min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=2)
    by_pose = _pairs(sequence.loop_candidates(sc["poses_init"], sequence.LoopClosureParams(**one)))
    by_look = _pairs(sequence.appearance_candidates(s4["loop_similarity"], both))
    assert got == sorted(set(by_pose) | set(by_look), key=lambda p: (p[1], p[0])) and len(got) == len(set(got))
    assert len(s4["loop_accepted"]) == len(got)
