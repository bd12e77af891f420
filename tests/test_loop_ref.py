"""The numpy statement of vus_stereo_pair_pose (tests/loop_ref.py) against planted truth -- conventions on exact data,
accuracy on integer pixels and disparities -- the edges its adversarial tables must really contain, and the host half
of the loop-closure path: sequence.loop_candidates and sequence.loop_closure_factors.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loop_ref as L

H, W = L.PLANTED_H, L.PLANTED_W
CAM = L.default_cam5(H, W)


def test_jacobian_matches_central_differences():
    """J = dr/dX [ [X]x | -I ] for the right perturbation T Exp(xi), xi = (omega, v)."""
    rng = np.random.default_rng(3)
    g = L.planted_pair(rng, 25, 0, L.PLANTED_POSE, H, W, quantise=False)
    P, u, v = L.points(g[0], g[1], g[2], CAM), g[3] + rng.normal(size=25), g[4] + rng.normal(size=25)
    T0 = L.retract(L.PLANTED_POSE, rng.normal(size=6) * 0.01)

    def resid(xi):
        return L.jacobians(L.transform(L.retract(T0, xi), P), u, v, CAM)[0]

    _, J = L.jacobians(L.transform(T0, P), u, v, CAM)
    h = 1e-6
    for q in range(6):
        e = np.zeros(6)
        e[q] = h
        num = (resid(e) - resid(-e)) / (2 * h)
        assert np.abs(num - J[:, :, q]).max() <= 1e-5 * max(1.0, np.abs(J[:, :, q]).max()), q


def test_exact_positions_recover_the_planted_pose():
    """Unquantised positions and disparities, no wrong match: every sample gives the pose up to rounding and the refit
    leaves it there.  Checks the conventions (P = R Q + t is T_a^-1 T_b) and every sign."""
    rng = np.random.default_rng(4)
    for c, pose in enumerate((L.PLANTED_POSE, L.pose12((-0.2, 0.1, -0.5), (-0.1, 0.3, 0.2)), L.IDENTITY12)):
        g = L.planted_pair(rng, 120, 0, pose, H, W, quantise=False)
        o = L.pair_pose(*g[:6], CAM, 2.0, 16, 11, c, 10)
        et, er = L.pose_error(o["T"], pose)
        print(f"exact data, pose {c}: {et:.3e} m, {er:.3e} rad, rss {o['rss']:.3e}, info {o['info']}")
        assert o["info"][:2] == (120, 0) and o["info"][2:] == (120, 120, 0, 10) and o["keep"].all()
        assert et <= 1e-8 and er <= 1e-8 and np.abs(o["T"] - pose).max() <= 1e-8
        assert o["rss"] <= 1e-12
        # the measurement is camera b's pose in camera a: a point of b maps into a
        Q = L.points(g[3], g[4], g[5], CAM)
        assert np.abs(L.points(g[0], g[1], g[2], CAM) - (Q @ o["T"][:9].reshape(3, 3).T + o["T"][9:])).max() <= 1e-8


def test_quantised_fixture():
    """Integer pixels and integer disparities >= 18 px, one wrong match in three: every wrong match is rejected, at
    least 60 % of the true ones are kept, and the pose error stays inside the fixture table's bounds (twice what this
    reference measured: 12.8 mm / 3.70e-3 rad at worst over the eight pairs)."""
    q = L.QUANTISED
    rng = np.random.default_rng(q["seed"])
    for c in range(q["n_pairs"]):
        g = L.planted_pair(rng, q["n_true"], q["n_wrong"], L.PLANTED_POSE, H, W)
        truth = g[6]
        assert min(g[2].min(), g[5].min()) >= 18
        o = L.pair_pose(*g[:6], CAM, L.THRESHOLD, q["n_hyp"], L.SEED, c, q["refine_iters"])
        et, er = L.pose_error(o["T"], L.PLANTED_POSE)
        print(f"quantised pair {c}: info {o['info']}, true kept {o['keep'][truth].mean():.3f}, wrong kept "
              f"{int(o['keep'][~truth].sum())}, error {1e3 * et:.2f} mm {er:.2e} rad")
        assert o["info"][4] == 0 and o["info"][5] == q["refine_iters"]
        assert not o["keep"][~truth].any()
        assert o["keep"][truth].mean() >= 0.6
        assert et <= q["bound_t_m"] and er <= q["bound_r_rad"], (c, et, er)
        assert o["info"][3] == o["keep"].sum() and np.allclose(o["JtJ"], o["JtJ"].T)


def test_best_is_the_first_maximum_and_samples_are_distinct():
    rng = np.random.default_rng(5)
    g = L.planted_pair(rng, 40, 40, L.PLANTED_POSE, H, W)
    o = L.pair_pose(*g[:6], CAM, L.THRESHOLD, 128, 9, 2, 0)
    assert o["info"][1] == int(np.argmax(o["counts"])) and o["info"][2] == o["counts"].max()
    assert o["info"][3] == o["info"][2] and o["info"][5] == 0             # no refit: the final set is the best model's
    h = L.mix(9 + 0x9E3779B9 * 3)
    for n in (3, 4, 5, 80):
        for k in range(200):
            ijl = L.sample(h, k, n)
            assert len(set(ijl)) == 3 and all(0 <= q < n for q in ijl)
    assert {L.sample(h, k, 3) for k in range(200)} >= {(0, 1, 2), (1, 2, 0), (2, 0, 1)}      # n - 2 = 1: l is what is left


def test_adversarial_tables_contain_their_edges():
    t, r = L.case("few")
    assert r["info"][:, 0].tolist() == [0, 1, 2, 3, 4, 3, 4]
    assert (r["info"][:3, 4] == 1).all() and (r["info"][:3, 1] == -1).all() and (r["match_idx_out"][:3] == -1).all()
    assert np.array_equal(r["T_ab"][:3], np.tile(L.IDENTITY12, (3, 1)))
    t, r = L.case("collinear")
    assert r["info"][:, 0].tolist() == [40, 12] and (r["info"][:, 4] == 2).all() and not r["JtJ"].any()
    t, r = L.case("no_disparity")
    assert r["info"][:, 0].tolist() == [0, 0, 5] and r["info"][2, 4] == 0 and (t["match_idx"][:2] >= 0).sum() == 60
    t, r = L.case("identical")
    assert (r["info"][:, 4] == 0).all() and np.array_equal(r["info"][:, 0], r["info"][:, 3])
    assert np.abs(r["T_ab"] - L.IDENTITY12).max() <= 1e-9 and r["rss"].max() <= 1e-12
    assert np.array_equal(r["match_idx_out"], t["match_idx"])
    t, r = L.case("pairing")
    a, b = t["pair_a"], t["pair_b"]
    assert (a > b).any() and (a == b).any() and (a < 0).any() and (b >= len(t["stereo_idx"])).any()
    assert np.bincount(np.concatenate([a[a >= 0], b[b < 4]]))[0] >= 3                     # frame 0 serves several pairs
    refused = (a == b) | (a < 0) | (b >= 4)
    assert (r["info"][refused, 4] == 1).all() and (r["info"][refused, 0] == 0).all()
    assert (t["match_idx"][refused] >= 0).any() and (r["match_idx_out"][refused] == -1).all()
    assert (r["info"][~refused, 0] == 40).all()
    t, r = L.case("bad_tables")
    K = t["match_idx"].shape[1]
    assert (t["kp_count"] > K).any() and (t["kp_count"] < 0).any()
    for tab in (t["match_idx"], t["stereo_idx"]):
        assert (tab >= K).any() and (tab < -1).any()
    assert r["info"][0, 0] > 20 and r["info"][0, 4] == 0 and r["info"][[1, 2, 4], 0].tolist() == [0, 0, 0]
    live = r["match_idx_out"] >= 0
    assert np.array_equal(r["match_idx_out"][live], t["match_idx"][live]) and (r["match_idx_out"][~live] == -1).all()
    t, r = L.case("planted_kp4096")
    assert r["info"][0, 0] == 4096 and r["info"][0, 4] == 0                                # every slot a candidate


# ----------------------------------------------------------------------------------------------------------------------
# sequence.loop_candidates

def lawn_mower(lanes=4, per_lane=8, spacing=0.4, lane_gap=0.6):
    """Camera poses of a survey pattern: lanes along x, alternate lanes flown backwards (the vehicle turns by 180 degrees
    about the vertical), camera looking down (its z axis is the world's -z)."""
    poses = []
    for l in range(lanes):
        for q in range(per_lane):
            x = q * spacing if l % 2 == 0 else (per_lane - 1 - q) * spacing
            yaw = 0.0 if l % 2 == 0 else np.pi
            Rz = L.rodrigues((0, 0, yaw))
            down = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
            poses.append(np.concatenate([(Rz @ down).reshape(-1), [x, l * lane_gap, 0.0]]))
    return np.array(poses)


def test_loop_candidates_on_a_lawn_mower_track():
    from visual_underwater_slam_amd.sequence import LoopClosureParams, loop_candidates
    P = lawn_mower()
    P[20, :9] = (L.rodrigues((0.9, 0, 0)) @ P[20, :9].reshape(3, 3)).reshape(-1)        # one camera tilted by 0.9 rad
    prm = LoopClosureParams(min_gap=5, radius_m=0.75, max_angle_rad=0.5, max_per_keyframe=2)
    a, b = loop_candidates(P, prm)
    assert a.dtype == np.int32 and b.dtype == np.int32 and len(a) == len(b) > 10
    a2, b2 = loop_candidates(P.copy(), prm)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    dist = np.linalg.norm(P[a, 9:] - P[b, 9:], axis=1)
    ang = np.arccos(np.clip((P[a][:, [2, 5, 8]] * P[b][:, [2, 5, 8]]).sum(1), -1, 1))
    assert (b - a >= 5).all() and (dist <= 0.75).all() and (ang <= 0.5).all()
    assert 20 not in a.tolist() and 20 not in b.tolist()                                  # the tilted one pairs with nothing
    assert np.bincount(b).max() == 2                                                       # the cap bites ...
    free = loop_candidates(P, LoopClosureParams(min_gap=5, radius_m=0.75, max_angle_rad=0.5, max_per_keyframe=99))
    assert np.bincount(free[1]).max() > 2                                                  # ... where more were near
    # order: by b, then by distance (ties: lower a); per b the kept ones are the nearest of all that qualify
    key = list(zip(b.tolist(), np.round(dist, 12).tolist(), a.tolist()))
    assert key == sorted(key)
    for bb in np.unique(b):
        allq = free[0][free[1] == bb]
        d_all = np.sort(np.linalg.norm(P[allq, 9:] - P[bb, 9:], axis=1))
        assert np.allclose(np.sort(dist[b == bb]), d_all[:2])
    # nothing qualifies: empty arrays, not an error
    none = loop_candidates(P, LoopClosureParams(min_gap=5, radius_m=0.01))
    assert len(none[0]) == 0 and none[0].dtype == np.int32
    assert len(loop_candidates(P, LoopClosureParams(min_gap=len(P)))[0]) == 0


# ----------------------------------------------------------------------------------------------------------------------
# sequence.loop_closure_factors

def fake_result(rng, n):
    """A PairPoses-shaped record on the host with well-conditioned normal matrices."""
    T = np.stack([L.pose12(rng.normal(size=3) * 0.3, rng.normal(size=3)) for _ in range(n)])
    A = rng.normal(size=(n, 40, 6))
    JtJ = np.einsum("nkp,nkq->npq", A, A) * 1e4
    info = np.zeros((n, 6), np.int32)
    info[:, 0], info[:, 3] = 100, 50
    return SimpleNamespace(T_ab=torch.from_numpy(T), JtJ=torch.from_numpy(JtJ), rss=torch.from_numpy(np.full(n, 94.0)),
                           info=torch.from_numpy(info), match_idx_out=None)


def test_loop_closure_factors_acceptance_scale_and_models():
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    from visual_underwater_slam_amd.sequence import LoopClosureParams, loop_closure_factors, loop_closure_measurements
    rng = np.random.default_rng(8)
    r = fake_result(rng, 6)
    info = r.info.numpy()
    info[1, 3] = 29                  # one inlier short
    info[2, 3] = 30                  # exactly min_inliers: accepted
    info[3, 4] = 3                   # a failed refit with many inliers
    info[4, 4] = 2
    r.rss[5] = 94.0 * 9              # residual scale 3
    pa, pb = np.array([0, 1, 2, 3, 4, 5], np.int32), np.array([10, 11, 12, 13, 14, 15], np.int32)
    prm = LoopClosureParams(min_inliers=30, sigma_px=1.0)
    acc, meas, cov, scale = loop_closure_measurements(r, prm)
    assert acc.tolist() == [True, False, True, False, False, True]
    # s = max(sigma_px, sqrt(rss / (2 n_in - 6))): 94 / 94 = 1 -> the floor; 94 / 54 -> 1.319; 9 * 94 / 94 -> 3
    assert scale[0] == 1.0 and np.isclose(scale[2], np.sqrt(94.0 / 54.0)) and np.isclose(scale[5], 3.0)
    assert LoopClosureParams(sigma_px=2.5).sigma_px == 2.5
    assert np.isclose(loop_closure_measurements(r, LoopClosureParams(sigma_px=2.5))[3][0], 2.5)
    for c in (0, 2, 5):
        assert np.allclose(cov[c] @ r.JtJ[c].numpy(), scale[c] ** 2 * np.eye(6), atol=1e-8)
    fs = loop_closure_factors(r, (pa, pb), prm)
    assert [f.keys() for f in fs] == [[X(0), X(10)], [X(2), X(12)], [X(5), X(15)]]
    for f, c in zip(fs, (0, 2, 5)):
        assert isinstance(f, gtsam.BetweenFactorPose3)
        assert f.measured().equals(gtsam.Pose3.from_flat12(r.T_ab[c].numpy()), 1e-12)
        assert np.allclose(f.noiseModel().sigmas(), np.sqrt(np.diag(cov[c])), rtol=1e-12)
        assert not isinstance(f.noiseModel(), gtsam.noiseModel.Robust)
    fr = loop_closure_factors(r, (torch.from_numpy(pa), torch.from_numpy(pb)), LoopClosureParams(robust=("Cauchy", 2.0)))
    assert len(fr) == 3 and all(isinstance(f.noiseModel(), gtsam.noiseModel.Robust) for f in fr)
    assert fr[0].noiseModel().robust().k == 2.0 and np.allclose(fr[0].noiseModel().sigmas(), fs[0].noiseModel().sigmas())
    # a normal matrix that cannot be inverted is no measurement
    r.JtJ[0] = 0.0
    assert loop_closure_measurements(r, prm)[0].tolist() == [False, False, True, False, False, True]


def test_body_P_sensor_conjugates_measurement_and_covariance():
    """measured = S T S^-1 (checked with Pose3.compose) and cov = Ad_S cov Ad_S^T, checked against the finite-difference
    push-forward of a camera-frame perturbation T Exp(xi) through the conjugation."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.sequence import (LoopClosureParams, adjoint_map, loop_closure_factors,
                                                     loop_closure_measurements)
    rng = np.random.default_rng(9)
    r = fake_result(rng, 2)
    S = gtsam.Pose3(gtsam.Rot3(L.rodrigues((0.4, -1.1, 0.7))), np.array([0.3, -0.2, 0.5]))
    prm = LoopClosureParams()
    _, meas_c, cov_c, _ = loop_closure_measurements(r, prm)
    acc, meas_b, cov_b, _ = loop_closure_measurements(r, prm, S)
    assert acc.all()
    for c in range(2):
        Tc = gtsam.Pose3.from_flat12(r.T_ab[c].numpy())
        M = S.compose(Tc).compose(S.inverse())
        assert meas_b[c].equals(M, 1e-12) and meas_c[c].equals(Tc, 1e-12)
        # body poses X = C S^-1: X_a^-1 X_b = S (C_a^-1 C_b) S^-1
        Ca = gtsam.Pose3.from_flat12(L.pose12(rng.normal(size=3), rng.normal(size=3)))
        Cb = Ca.compose(Tc)
        assert Ca.compose(S.inverse()).between(Cb.compose(S.inverse())).equals(M, 1e-10)
        h, Jf = 1e-6, np.zeros((6, 6))
        for q in range(6):
            e = np.zeros(6)
            e[q] = h
            f = lambda xi: gtsam.Pose3.Logmap(M.between(S.compose(Tc.retract(xi)).compose(S.inverse())))
            Jf[:, q] = (f(e) - f(-e)) / (2 * h)
        assert np.abs(Jf - adjoint_map(S)).max() <= 1e-8
        push = Jf @ cov_c[c] @ Jf.T
        assert np.abs(cov_b[c] - push).max() <= 1e-6 * np.abs(push).max()
    fb = loop_closure_factors(r, (np.array([0, 1]), np.array([7, 9])), prm, S)
    assert np.allclose(fb[1].noiseModel().sigmas(), np.sqrt(np.diag(cov_b[1]))) and fb[1].measured().equals(meas_b[1], 1e-12)
    assert not np.allclose(fb[1].noiseModel().sigmas(), np.sqrt(np.diag(cov_c[1])), rtol=1e-3)
