"""What the appearance-retrieval tests add to the closed track of tests/loop_scene.py: an odometry estimate that has drifted
ten times as far (1.8 m at the last keyframe, beyond LoopClosureParams.radius_m, so pose proximity cannot propose the
revisit), and the similarity matrix of a front-end result by the numpy statement.  Test infrastructure only (a plain module,
not a conftest): used by tests/test_retrieval_ref.py and tests/test_loop_retrieval_sequence_gpu.py."""
import numpy as np

import loop_ref as L
import loop_scene as S
import retrieval_ref as R

DRIFT_FACTOR = 10
NO_GROUND = 4            # the keyframe at the far end: it shares no ground with the last keyframe either
LAST = S.N_KF - 1


def poses_far_drifted(gt):
    """loop_scene.poses_drifted with ten times the drift: 20 cm and 40 mrad of yaw per keyframe."""
    out = []
    for k, T in enumerate(gt):
        R3 = L.rodrigues((0.0, 0.0, 0.004 * DRIFT_FACTOR * k)) @ T[:9].reshape(3, 3)
        out.append(np.concatenate([R3.reshape(-1), T[9:] + np.array([0.016, -0.012, 0.002]) * (DRIFT_FACTOR * k)]))
    return np.array(out)


def similarity_ref(desc, kp_count, n_kf, top, max_dist, min_gap=0):
    """keyframe_similarity's matrix by the numpy statement: left images, S[b, a] for a <= b - min_gap."""
    img = 2 * np.arange(n_kf)
    return R.keyframe_similarity(desc, kp_count, img, img, np.maximum(np.arange(n_kf) - min_gap + 1, 0), top, max_dist)


def check_ranking(Sm, prm, candidates):
    """The assertions both front ends must meet on the track: keyframe 0 is the best of 0..4 for the last keyframe and is
    proposed; keyframe 4, which shares no ground with it, is not."""
    assert int(np.argmax(Sm[LAST, :NO_GROUND + 1])) == S.REVISIT[0], Sm[LAST]
    assert Sm[LAST, S.REVISIT[0]] >= prm.appearance_min_score, Sm[LAST]
    assert Sm[LAST, NO_GROUND] < prm.appearance_min_score, Sm[LAST]
    pairs = list(zip(candidates[0].tolist(), candidates[1].tolist()))
    assert S.REVISIT in pairs, pairs
    assert (NO_GROUND, LAST) not in pairs, pairs
