"""The numpy statement of vus_stereo_pair_bundle (tests/pair_bundle_ref.py) against things that do not share its code:
central differences, the dense normal equations of poses and points together, a planted pose, and the accuracy the
two-view refit was built for (no GPU needed)."""
import numpy as np

import loop_ref as L
import pair_bundle_ref as B

H, W = 360, 640
CAM = L.default_cam5(H, W)
TRUTH = L.pose12([0.02, 0.44, -0.03], [0.35, -0.05, 0.1])


def stacked_residual(T12, p, za, zb, w):
    """The whitened residual vector of all points, [n * 6]."""
    ra, rb, _, _, _, _ = B.residuals(T12, p, za, zb, CAM, w)
    s = np.sqrt(w)
    return np.concatenate([ra * s, rb * s], 1).reshape(-1)


def scene(seed, n=5, quantise=False, zrange=(2.5, 4.2)):
    rng = np.random.default_rng(seed)
    g = L.planted_pair(rng, n, 0, TRUTH, H, W, CAM, zrange=zrange, quantise=quantise)
    za, zb = np.stack(g[:3], 1), np.stack(g[3:6], 1)
    return rng, za, zb


def test_jacobians_equal_central_differences():
    rng, za, zb = scene(1, n=6)
    w = B.weights(0.5, 0.12)
    T0 = L.retract(TRUTH, rng.normal(size=6) * 0.01)
    p = L.points(za[:, 0], za[:, 1], za[:, 2], CAM) + rng.normal(size=(6, 3)) * 0.01
    bl = B.blocks(T0, p, za, zb, CAM, w)
    h = 1e-6
    for q in range(6):
        e = np.zeros(6)
        e[q] = h
        Xp, Xm = L.transform(L.retract(T0, e), p), L.transform(L.retract(T0, -e), p)
        num = (B.project(Xp, CAM)[0] - B.project(Xm, CAM)[0]) / (2 * h)
        assert np.abs(num - bl["Jt"][:, :, q]).max() <= 1e-6 * np.abs(bl["Jt"]).max(), q
    for q in range(3):
        e = np.zeros(3)
        e[q] = h
        num_a = (B.project(p + e, CAM)[0] - B.project(p - e, CAM)[0]) / (2 * h)
        num_b = (B.project(L.transform(T0, p + e), CAM)[0] - B.project(L.transform(T0, p - e), CAM)[0]) / (2 * h)
        assert np.abs(num_a - bl["Ja"][:, :, q]).max() <= 1e-6 * np.abs(bl["Ja"]).max(), q
        assert np.abs(num_b - bl["Jp"][:, :, q]).max() <= 1e-6 * np.abs(bl["Jp"]).max(), q


def test_reduced_system_is_the_schur_complement_of_the_dense_normal_equations():
    n = 5
    rng, za, zb = scene(2, n=n)
    w = B.weights(0.5, 0.12)
    T0 = L.retract(TRUTH, rng.normal(size=6) * 0.003)
    p = L.points(za[:, 0], za[:, 1], za[:, 2], CAM) + rng.normal(size=(n, 3)) * 0.003
    # the dense Jacobian of the whitened residuals by central differences, columns (pose 6, points 3 n)
    h, cols = 1e-6, []
    for q in range(6):
        e = np.zeros(6)
        e[q] = h
        cols.append((stacked_residual(L.retract(T0, e), p, za, zb, w) - stacked_residual(L.retract(T0, -e), p, za, zb, w)) / (2 * h))
    for i in range(n):
        for q in range(3):
            d = np.zeros((n, 3))
            d[i, q] = h
            cols.append((stacked_residual(T0, p + d, za, zb, w) - stacked_residual(T0, p - d, za, zb, w)) / (2 * h))
    J = np.stack(cols, 1)
    r = stacked_residual(T0, p, za, zb, w)
    N, b = J.T @ J, J.T @ r
    Npp_inv = np.linalg.inv(N[6:, 6:])
    S_dense = N[:6, :6] - N[:6, 6:] @ Npp_inv @ N[6:, :6]
    g_dense = b[:6] - N[:6, 6:] @ Npp_inv @ b[6:]
    red = B.reduced(T0, p, za, zb, CAM, w, gate=1e6)
    assert red["active"].all()
    assert np.abs(red["S"] - S_dense).max() <= 1e-6 * np.abs(S_dense).max()
    assert np.abs(red["g"] - g_dense).max() <= 1e-6 * max(np.abs(g_dense).max(), np.abs(b).max())
    assert abs(red["chi2"] - r @ r) <= 1e-12 * (r @ r)
    # the full step of the dense system is the reduced step and the back-substitution
    full = np.linalg.solve(N, b)
    delta = L.cholesky_solve(red["S"], red["g"])
    step = red["yp"] - np.einsum("nrc,c->nr", red["Y"], delta)
    assert np.abs(delta - full[:6]).max() <= 1e-5 * np.abs(full[:6]).max()
    assert np.abs(step.reshape(-1) - full[6:]).max() <= 1e-5 * np.abs(full[6:]).max()


def test_exact_observations_recover_the_planted_pose():
    rng, za, zb = scene(3, n=150)
    start = L.retract(TRUTH, np.array([0.004, -0.006, 0.005, 0.02, -0.015, 0.01]))
    o = B.pair_bundle(za[:, 0], za[:, 1], za[:, 2], zb[:, 0], zb[:, 1], zb[:, 2], CAM, start, False, 0.5, 0.12, 1e3, 10)
    assert o["info"][3] == B.STATUS_OK and o["info"][2] == 150
    et, er = L.pose_error(o["T"], TRUTH)
    print(f"exact observations: translation {et:.2e} m, rotation {er:.2e} rad, chi2 {o['chi2']:.2e}")
    assert et <= 1e-9 and er <= 1e-9
    assert np.abs(o["points"] - L.points(za[:, 0], za[:, 1], za[:, 2], CAM)).max() <= 1e-9


def noisy_pair(seed, sigma_d=0.12, zrange=(3.99, 4.01), n_true=300, n_wrong=150, moved=0.1):
    """The issue's setting: exact projections, left pixel positions rounded to integers, Gaussian disparity noise, and a
    tenth of b's disparities moved by +-3 px.  Returns (x1, y1, d1, x2, y2, d2, truth, moved)."""
    rng = np.random.default_rng(seed)
    x1, y1, d1, x2, y2, d2, truth = L.planted_pair(rng, n_true, n_wrong, TRUTH, H, W, CAM, zrange=zrange, quantise=False)
    x1, y1, x2, y2 = (np.round(v) for v in (x1, y1, x2, y2))
    d1 = d1 + rng.normal(size=len(d1)) * sigma_d
    d2 = d2 + rng.normal(size=len(d2)) * sigma_d
    mv = rng.random(len(d2)) < moved
    d2 = d2 + np.where(mv, rng.choice([-3.0, 3.0], len(d2)), 0.0)
    return x1, y1, d1, x2, y2, d2, truth, mv


def test_two_view_refit_halves_the_translation_error_of_the_left_only_refit():
    """640 x 360, plane at 3.99-4.01 m, 300 true + 150 wrong matches, 10 % of b's disparities moved by +-3 px, disparity
    noise 0.12 px, 6 seeds: the median translation error of the two-view refit is at most half that of the left-only
    refit it follows, and no moved-disparity point is active at the end."""
    left, two = [], []
    for seed in range(6):
        x1, y1, d1, x2, y2, d2, truth, mv = noisy_pair(100 + seed)
        one = L.pair_pose(x1, y1, d1, x2, y2, d2, CAM, 2.0, 256, 20261019, 0, 10)
        assert one["info"][4] == 0
        k = one["keep"]
        o = B.pair_bundle(x1[k], y1[k], d1[k], x2[k], y2[k], d2[k], CAM, one["T"], False, 0.5, 0.12, 4.0, 10)
        assert o["info"][3] == B.STATUS_OK
        left.append(L.pose_error(one["T"], TRUTH)[0])
        two.append(L.pose_error(o["T"], TRUTH)[0])
        passed, still = int(mv[k].sum()), int((mv[k] & o["keep"]).sum())
        wrong = int((~truth[k] & o["keep"]).sum())
        print(f"seed {seed}: left-only {1e3 * left[-1]:.1f} mm, two-view {1e3 * two[-1]:.1f} mm; stage one passed {passed} moved "
              f"disparities, {still} active at the end; {int(o['keep'].sum())} of {int(k.sum())} active, {wrong} wrong matches")
        assert passed > 0 and still == 0
    ml, mt = float(np.median(left)), float(np.median(two))
    print(f"median translation error: left-only {1e3 * ml:.1f} mm, two-view {1e3 * mt:.1f} mm, ratio {mt / ml:.2f}")
    assert mt <= 0.5 * ml


def test_fixtures_are_certified_and_statuses_are_what_they_say():
    t, T_in, info_in, ref = B.explicit_case("few")
    # n = 3 with one point outside the gate: two active points do not fix a pose (status 3 by count, before any pivot)
    assert ref["info"][:, 0].tolist() == [0, 1, 2, 3, 4] and ref["info"][:, 3].tolist() == [1, 1, 1, 3, 0]
    assert ref["info"][3, 1] == 2 and np.array_equal(ref["T_ab"][3], T_in[3])
    t, T_in, info_in, ref = B.explicit_case("gated")
    assert ref["info"][:, 3].tolist() == [B.STATUS_SOLVE, B.STATUS_OK]
    assert np.array_equal(ref["T_ab"][0], T_in[0]) and not ref["S"][0].any() and (ref["match_idx_out"][0] == -1).all()
    t, T_in, info_in, ref = B.explicit_case("passed")
    assert ref["info"][:, 3].tolist() == [B.STATUS_PASSED, B.STATUS_OK]
    assert np.array_equal(ref["T_ab"][0], T_in[0]) and not ref["points"][0].any()
    t, T_in, info_in, ref = B.case("planted_kp257")
    live = ref["info"][:, 3] == 0
    assert live.all() and (ref["info"][:, 2] >= 50).all() and (ref["info"][:, 4] == B.ITERS).all()
    # the points of the active slots are the only non-zero ones
    assert np.array_equal(ref["points"].any(-1), ref["match_idx_out"] >= 0)


def test_closure_parameters_and_the_whitened_covariance_rule():
    """LoopClosureParams' new arguments and their defaults, and loop_closure_measurements on a PairBundle filled from the
    reference: cov = s^2 S^-1, s = max(1, sqrt(chi2 / (3 n - 6))), min_inliers counted on the final active points."""
    import dataclasses
    import pytest
    import torch
    from visual_underwater_slam_amd.frontend import PairBundle
    from visual_underwater_slam_amd.sequence import LoopClosureParams, loop_closure_measurements
    prm = LoopClosureParams()
    assert (prm.refit, prm.sigma_uv_px, prm.sigma_disp_px, prm.gate_sigma) == ("left", 0.5, None, 4.0)
    assert (prm.disparity_sigma(False), prm.disparity_sigma(True)) == (0.6, 0.12)
    assert LoopClosureParams(sigma_disp_px=0.3).disparity_sigma(True) == 0.3
    assert LoopClosureParams(refit="stereo", long_span=4).refit == "stereo"
    assert "refit" not in [f.name for f in dataclasses.fields(prm)]       # init-only, like long_span: the fields stay as they were
    for bad in ("right", "", "Left", None):
        with pytest.raises(ValueError, match="refit"):
            LoopClosureParams(refit=bad)
    t, T_in, info_in, ref = B.case("planted_kp257")
    d = torch.from_numpy
    res = PairBundle(T_ab=d(ref["T_ab"]), S=d(ref["S"]).reshape(-1, 6, 6), chi2=d(ref["chi2"]), points=d(ref["points"]),
                     info=d(ref["info"]), match_idx_out=d(ref["match_idx_out"]))
    n = ref["info"][:, 2]
    acc, meas, cov, scale = loop_closure_measurements(res, LoopClosureParams(refit="stereo", min_inliers=int(n.min())))
    assert acc.all()
    for c in range(len(n)):
        s = max(1.0, float(np.sqrt(ref["chi2"][c] / (3 * n[c] - 6))))
        assert scale[c] == s and np.allclose(cov[c], s * s * np.linalg.inv(ref["S"][c].reshape(6, 6)), rtol=1e-12, atol=0.0)
        assert np.array_equal(meas[c].flat12(), ref["T_ab"][c])
    acc = loop_closure_measurements(res, LoopClosureParams(refit="stereo", min_inliers=int(n.min()) + 1))[0]
    assert acc.tolist() == (n > n.min()).tolist()
    # a passed-through pair (status 4) and a failed one (3) are not measurements
    bad = dataclasses.replace(res, info=d(np.array([[144, 0, 0, 4, 0, 0], [98, 97, 0, 3, 2, 0]], np.int32)))
    assert not loop_closure_measurements(bad, LoopClosureParams(refit="stereo", min_inliers=0))[0].any()
