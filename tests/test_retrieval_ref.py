"""Loop-closure candidates by appearance, on the CPU: the two forms of the numpy statement of vus_keyframe_similarity
(tests/retrieval_ref.py: popcount and +-1 matrix product) agree; sequence.appearance_candidates, the union with the pose
candidates and the new LoopClosureParams fields do what they say; and on the closed track of tests/loop_scene.py the score
ranks the revisit first and never proposes the keyframe without common ground, while pose proximity on a far-drifted odometry
misses the revisit."""
import numpy as np
import pytest

import loop_scene as S
import retrieval_ref as R
import retrieval_scene as RS


def _random_desc(rng, n_img, K):
    return rng.integers(0, 2**63, size=(n_img, K, 4), dtype=np.int64).view(np.uint64) ^ \
        (rng.integers(0, 2, size=(n_img, K, 4), dtype=np.uint64) << np.uint64(63))


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


def test_popcount_and_matmul_forms_agree_on_random_descriptors():
    rng = np.random.default_rng(31)
    K = 150
    desc = _random_desc(rng, 6, K)
    for i in range(1, 6):                            # image i = image i-1 permuted, with up to 40 flipped bits per descriptor
        perm = rng.permutation(K)
        for j in range(K):
            desc[i, j] = _flip(desc[i - 1, perm[j]], rng.integers(0, 256, size=j % 41))
    kc = np.array([K, 97, 0, -3, K + 9, 33], np.int32)
    q = [0, 1, 2, 3, 4, 5, 1, 9, -1]
    t = [5, 4, 3, 2, 1, 0, 0, 6]
    lim = [8, 9, 3, 0, -2, 5, 1, 8, 8]
    for top, max_dist in ((K, 35), (64, 20), (1, 256), (100, 0)):
        a = R.keyframe_similarity(desc, kc, q, t, lim, top, max_dist, form="popcount")
        b = R.keyframe_similarity(desc, kc, q, t, lim, top, max_dist, form="matmul")
        assert a.dtype == np.int32 and a.shape == (9, 8) and np.array_equal(a, b), (top, max_dist)
        assert (a[3] == 0).all() and (a[4] == 0).all() and (a[7:] == 0).all() and (a[:, 7] == 0).all()   # limits, bad images
        assert (a[2] == 0).all() and (a[:, 2] == 0).all() and (a[:, 3] == 0).all()                        # empty images
        assert a[1, 4] == min(97, top) and a[0, 5] == min(K, top)                                          # the self pairs
        assert a[6, 0] == a[1, 0] and a[6, 1:].sum() == 0                                                  # a repeated image; limit 1
    full = R.keyframe_similarity(desc, kc, q, t, None, K, 35)
    assert 0 < full[1, 5] < 97 and full[4, 7] == 0      # image 1 is image 0 with up to 40 flipped bits; no limit, bad image


@pytest.mark.parametrize("max_dist", [0, 35, 255, 256])
def test_forms_agree_on_planted_neighbours_around_the_bound(max_dist):
    rng = np.random.default_rng(32 + max_dist)
    K = 64
    desc = _random_desc(rng, 2, K)
    want = 0
    for i in range(K):                               # query i's only near neighbour lies exactly d bits away
        d = max(0, min(256, max_dist + (i % 5) - 2))
        desc[0, i] = _flip(desc[1, (5 * i) % K], rng.permutation(256)[:d])
        want += d <= max_dist
    kc = np.array([K, K], np.int32)
    a = R.keyframe_similarity(desc, kc, [0, 1], [1, 0], None, K, max_dist, form="popcount")
    b = R.keyframe_similarity(desc, kc, [0, 1], [1, 0], None, K, max_dist, form="matmul")
    assert np.array_equal(a, b)
    if max_dist < 100:                               # random descriptors lie ~128 bits apart: only the planted ones count
        assert a[0, 0] == want, (a, want)
    else:
        assert a[0, 0] >= want
    if max_dist == 256:
        assert (a == K).all()


def test_extreme_descriptors():
    desc = np.zeros((2, 4, 4), np.uint64)
    desc[1] = np.uint64(0xFFFFFFFFFFFFFFFF)          # distance 256: dot -256
    kc = np.array([4, 4], np.int32)
    for form in ("popcount", "matmul"):
        assert R.keyframe_similarity(desc, kc, [0], [1], None, 4, 255, form=form)[0, 0] == 0
        assert R.keyframe_similarity(desc, kc, [0], [1], None, 4, 256, form=form)[0, 0] == 4
        assert R.keyframe_similarity(desc, kc, [0], [0], None, 3, 0, form=form)[0, 0] == 3


def _params(**kw):
    from visual_underwater_slam_amd.sequence import LoopClosureParams
    return LoopClosureParams(**kw)


def test_appearance_candidates_on_hand_made_matrices():
    from visual_underwater_slam_amd.sequence import appearance_candidates
    Sm = np.array([[9, 0, 0, 0, 0, 0],
                   [50, 9, 0, 0, 0, 0],
                   [40, 40, 9, 0, 0, 0],             # a tie: the lower a first
                   [29, 30, 31, 9, 0, 0],            # 29 is below min_score
                   [60, 70, 70, 80, 9, 0],           # four eligible, the two best kept: 80, then 70 at the lower a
                   [0, 0, 0, 0, 0, 9]], np.int32)
    pa, pb = appearance_candidates(Sm, _params(min_gap=1, max_per_keyframe=2))
    assert pa.dtype == np.int32 and pb.dtype == np.int32
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 1), (0, 2), (1, 2), (2, 3), (1, 3), (3, 4), (1, 4)]
    pa, pb = appearance_candidates(Sm, _params(min_gap=2, max_per_keyframe=3))
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 2), (1, 3), (1, 4), (2, 4), (0, 4)]
    pa, pb = appearance_candidates(Sm, _params(min_gap=1, max_per_keyframe=1, appearance_min_score=41))
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 1), (3, 4)]
    pa, pb = appearance_candidates(Sm, _params(min_gap=0, max_per_keyframe=1, appearance_min_score=0))   # the self pair is eligible
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 0), (0, 1), (0, 2), (2, 3), (3, 4), (5, 5)]
    for prm in (_params(min_gap=1, max_per_keyframe=0), _params(min_gap=6), _params(min_gap=1, appearance_min_score=81)):
        pa, pb = appearance_candidates(Sm, prm)      # nothing kept, no keyframe far enough back, nothing scores enough
        assert len(pa) == 0 and len(pb) == 0 and pa.dtype == np.int32 and pb.dtype == np.int32
    # what lies above the diagonal band is never read
    poisoned = Sm.copy()
    poisoned[np.triu_indices(6, 0)] = 999
    pa2, pb2 = appearance_candidates(poisoned, _params(min_gap=1, max_per_keyframe=2))
    assert list(zip(pa2.tolist(), pb2.tolist())) == [(0, 1), (0, 2), (1, 2), (2, 3), (1, 3), (3, 4), (1, 4)]


def test_union_of_the_two_candidate_sets():
    from visual_underwater_slam_amd.sequence import union_candidates
    pose = (np.array([0, 2, 1], np.int32), np.array([7, 7, 9], np.int32))
    look = (np.array([0, 2, 0, 1], np.int32), np.array([9, 7, 6, 9], np.int32))
    pa, pb = union_candidates(pose, look)
    assert pa.dtype == np.int32 and pb.dtype == np.int32
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 6), (0, 7), (2, 7), (0, 9), (1, 9)]
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    pa, pb = union_candidates(none, none)
    assert len(pa) == 0 and len(pb) == 0 and pa.dtype == np.int32
    pa, pb = union_candidates(none, look)
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 6), (2, 7), (0, 9), (1, 9)]


def test_params_defaults_keep_pose_mode_and_a_bad_mode_raises():
    prm = _params()
    assert prm.candidates == "pose"
    assert (prm.appearance_top, prm.appearance_max_distance, prm.appearance_min_score) == (512, 35, 30)
    import dataclasses
    names = [f.name for f in dataclasses.fields(prm)]
    assert names[-4:] == ["candidates", "appearance_top", "appearance_max_distance", "appearance_min_score"]   # appended
    assert names[0] == "min_gap" and names[names.index("candidates") - 1] == "robust"
    for mode in ("pose", "appearance", "both"):
        assert _params(candidates=mode).candidates == mode
    for bad in ("looks", "", "Pose", None):
        with pytest.raises(ValueError, match="candidates"):
            _params(candidates=bad)


@pytest.fixture(scope="module")
def oracle_front():
    from oracle import chain
    from visual_underwater_slam_amd import sequence, synth
    gt = S.poses_gt()
    fe = chain.frontend(synth.scene_frames(gt, S.H, S.W), S.KP, **sequence.SEQUENCE_PARAMS)
    return gt, fe


def test_score_ranks_the_revisit_on_the_closed_track(oracle_front):
    from visual_underwater_slam_amd.sequence import appearance_candidates
    gt, fe = oracle_front
    prm = _params(candidates="appearance")
    assert prm.min_gap == 5
    Sm = RS.similarity_ref(fe["desc"], fe["kp_count"], S.N_KF, prm.appearance_top, prm.appearance_max_distance)
    print(Sm)
    RS.check_ranking(Sm, prm, appearance_candidates(Sm, prm))
    assert (np.triu(Sm, 1) == 0).all() and (np.diag(Sm) == np.minimum(fe["kp_count"][::2], prm.appearance_top)).all()
    # the matrix keyframe_similarity hands run_sequence (min_gap applied on the device) proposes the same pairs
    Sg = RS.similarity_ref(fe["desc"], fe["kp_count"], S.N_KF, prm.appearance_top, prm.appearance_max_distance, prm.min_gap)
    assert np.array_equal(Sg, np.tril(Sm, -prm.min_gap))
    for x, y in zip(appearance_candidates(Sm, prm), appearance_candidates(Sg, prm)):
        assert np.array_equal(x, y)


def test_pose_proximity_misses_the_revisit_once_the_odometry_has_drifted_far():
    from visual_underwater_slam_amd.sequence import loop_candidates
    gt = S.poses_gt()
    prm = _params()
    near = loop_candidates(S.poses_drifted(gt), prm)
    far_poses = RS.poses_far_drifted(gt)
    assert np.linalg.norm(far_poses[-1, 9:] - gt[-1, 9:]) > prm.radius_m
    far = loop_candidates(far_poses, prm)
    assert S.REVISIT in list(zip(near[0].tolist(), near[1].tolist()))
    assert S.REVISIT not in list(zip(far[0].tolist(), far[1].tolist()))
