"""Robust stereo factors on the MI355X: the `_robust` kernels stage by stage against the numpy reference
(tests/robust_ref.py), the Gaussian limit against today's entry points and the oracle, the LM bookkeeping (quadratic
value in the linear slots, rho in the nonlinear ones) against the reference LM, outlier recovery, the gtsam drop-in
path, the navigation graph and the landmark-sharded solver."""
import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth, ba_pack
from conftest import same_lm_trajectory
import robust_ref

pytestmark = pytest.mark.gpu

# (kind, k): VUS_LOSS_* with parameters in whitened units (sigma = 10 px; inlier residuals are ~0.17, the injected
# outliers 5..30)
LOSSES = {"huber": (1, 1.345), "cauchy": (2, 2.3849), "tukey": (3, 4.6851), "geman_mcclure": (4, 2.0),
          "welsch": (5, 2.9846)}
# Outlier recovery on ba_sequence(200, 3000, 300) with 3 % injected outliers (seed 5), bounds set from the measured run
# with a >= 3x margin on both sides.  Measured RMS translation error against ground truth: Gaussian 0.0523 m, Cauchy
# 0.00287 m, Huber 0.00268 m.  Final Cauchy weights: 99th percentile of the overrulable outliers (_constrained) 0.096,
# 1st percentile of the inliers 0.981.
RMS_BOUND = 0.012             # m: the Gaussian solve is pulled off by more than this, the Cauchy / Huber solves are not
W_OUTLIER_P99 = 0.3           # 99th percentile of the overrulable outliers' final weights (Cauchy)
W_INLIER_P01 = 0.94           # 1st percentile of the inliers' final weights (Cauchy): 1 - w within 3x of the measured
# navigation graph (nav_sequence(16, 400, 80), 3 % outliers), measured RMS translation error: Gaussian 0.068 m, Cauchy
# 0.0065 m -- one bound with >= 3x margin on both sides
NAV_RMS_BOUND = 0.021


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(seq, loss, n_kf=None, **kw):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    n_kf = n_kf or len(seq["poses_gt"])
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, len(seq["points_gt"]), seq["K"],
                           seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1],
                           prior_sigmas=seq["prior_sigmas"][None], loss=loss, **kw)
    return prob, StereoBASolver(prob)


def _ref(oracle, prob, seq, kind, k):
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    return robust_ref.RobustBA(oracle, pk, seq["K"], seq["sigma"], kind, k,
                               (np.array([0]), seq["poses_gt"][:1], seq["prior_sigmas"][None]))


def _stage_sequence():
    seq = synth.ba_sequence(60, 900, 150)
    mask = synth.inject_outliers(seq, 0.05, (50.0, 300.0))
    seq["points_init"] = seq["points_init"].copy()
    seq["points_init"][7, 2] = -1.0          # landmark 7 behind every camera that sees it: cheirality observations
    return seq, mask


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_robust_stages_match_the_reference(gpu, oracle, name):
    kind, k = LOSSES[name]
    seq, mask = _stage_sequence()
    prob, sv = _problem(seq, (kind, k))
    R = _ref(oracle, prob, seq, kind, k)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv.linearize(poses, points)
    lin = R.linearize(seq["poses_init"], seq["points_init"])
    got = {"W": sv.W, "V": sv.V, "gl": sv.gl, "Hpp": sv.Hpp, "gp": sv.gp}
    for key, v in got.items():
        assert relerr(v.cpu().numpy(), lin[key]) <= 1e-11, key
    assert float(sv.scal[0]) == pytest.approx(lin["err"], rel=1e-11)
    nl_err = R.error(seq["poses_init"], seq["points_init"])
    assert sv.error(poses, points) == pytest.approx(nl_err, rel=1e-11)
    assert not np.isclose(lin["err"], nl_err, rtol=1e-6)       # the linear and the nonlinear error differ here
    # one trial: GPU step (its own solve), then both outputs of eval_step against the reference at that step
    sv.linearize(poses, points)
    sv.schur(1e-3); sv.band_solve(); sv.backsub()
    sv.eval_step(poses, points)
    dp, dl = sv.dp.cpu().numpy(), sv.dl.cpu().numpy()
    npo, npt, lin1, new1 = R.eval_step(seq["poses_init"], seq["points_init"], dp, dl)
    assert float(sv.scal[1]) == pytest.approx(lin1, rel=1e-11)
    assert float(sv.scal[2]) == pytest.approx(new1, rel=1e-11)
    assert relerr(sv.new_poses.cpu().numpy(), npo) <= 1e-12
    # weights in the input row order (ba_sequence rows) against the reference's L-order weights
    w = sv.stereo_weights(poses, points).cpu().numpy()
    perm = prob.pk["perm"].cpu().numpy().astype(np.int64)
    want = np.empty_like(w)
    want[perm] = lin["w"]
    assert np.abs(w - want).max() <= 1e-11
    cheir = seq["obs_point"] == 7
    assert cheir.any() and np.all(w[cheir] < 1.0)
    if name == "tukey":
        assert np.all(w[cheir] == 0.0)


def test_gaussian_limit_equals_todays_entry_points(gpu, oracle):
    """Huber with k = 1e12: every w = 1, the robust kernels compute what the Gaussian ones do (to 1e-14), and the full LM
    through them walks the oracle's Gaussian trajectory."""
    seq, _ = _stage_sequence()
    seq["points_init"] = synth.ba_sequence(60, 900, 150)["points_init"]
    prob_g, sv_g = _problem(seq, None)
    prob_h, sv_h = _problem(seq, ("huber", 1e12))
    assert not prob_g.robust and prob_h.robust
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv_g.linearize(poses, points)
    sv_h.linearize(poses, points)
    for a, b in ((sv_h.W, sv_g.W), (sv_h.V, sv_g.V), (sv_h.gl, sv_g.gl), (sv_h.Hpp, sv_g.Hpp), (sv_h.gp, sv_g.gp),
                 (sv_h.scal[:1], sv_g.scal[:1])):
        assert relerr(a.cpu().numpy(), b.cpu().numpy()) <= 1e-14
    assert sv_h.error(poses, points) == pytest.approx(sv_g.error(poses, points), rel=1e-14)
    assert np.all(sv_h.stereo_weights(poses, points).cpu().numpy() == 1.0)
    oposes, opoints, orep = oracle.ba_lm_optimize(
        oracle.BAProblem({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in prob_h.pk.items()}, seq["K"], seq["sigma"],
                         (np.array([0], np.int32), seq["poses_gt"][:1], seq["prior_sigmas"][None])),
        prob_h.band, seq["poses_init"], seq["points_init"])
    p, pt, rep = sv_h.optimize(poses, points)
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    assert relerr(p.cpu().numpy(), oposes) < 1e-9 and relerr(pt.cpu().numpy(), opoints) < 1e-8


@pytest.mark.parametrize("name", ("huber", "cauchy"))
def test_robust_lm_walks_the_reference_lm(gpu, oracle, name):
    """The GPU LM and the numpy reference LM take the same trials and lambdas: a kernel that reported rho in a linear
    slot (or the quadratic in a nonlinear one) changes the gain ratio and with it the trajectory.  Cauchy's final state
    agrees to 1e-8; Huber's only to round-off amplified by a flat valley: its linear tails leave the outliers' landmarks
    weakly determined, LM stops at relativeErrorTol = 1e-5 short of the optimum, and two exact solves of the same trial
    system (the reference's LU and Schur forms) already differ there by ~2e-7 relative in the poses.  The final error
    agrees to 1e-9 for both."""
    kind, k = LOSSES[name]
    seq = synth.ba_sequence(12, 300, 60)
    mask = synth.inject_outliers(seq, 0.10, (50.0, 300.0), seed=11)
    assert mask.sum() >= 50
    prob, sv = _problem(seq, (kind, k))
    R = _ref(oracle, prob, seq, kind, k)
    rposes, rpoints, rrep = R.lm(seq["poses_init"], seq["points_init"])
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    assert rrep["outer"] >= 3
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    e_err, e_p, e_pt = (abs(rep.final_error / rrep["final_error"] - 1), relerr(poses.cpu().numpy(), rposes),
                        relerr(points.cpu().numpy(), rpoints))
    print(f"robust LM {name}: outer {rep.outer} tries {rep.tries}; final error {e_err:.2g}, poses {e_p:.2g}, points {e_pt:.2g}")
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    # measured: Cauchy 1e-10 / 4e-10, Huber 5e-7 / 1.1e-5 (poses / points)
    tol_p, tol_pt = (1e-8, 1e-8) if name == "cauchy" else (5e-6, 1e-4)
    assert e_err <= 1e-9 and e_p <= tol_p and e_pt <= tol_pt


def _constrained(seq, mask):
    """injected outliers the rest of the graph can overrule: their landmark has >= 3 observations and no other outlier
    (an outlier on a landmark seen once or twice is as consistent as the inlier beside it)"""
    ol = seq["obs_point"]
    n = np.bincount(ol)
    n_out = np.bincount(ol, weights=mask.astype(np.float64), minlength=len(n))
    return mask & (n[ol] >= 3) & (n_out[ol] <= 1)


def _rms_t(poses, seq):
    return float(np.sqrt(np.mean(np.sum((np.asarray(poses)[:, 9:] - seq["poses_gt"][:, 9:]) ** 2, 1))))


def _recovery_sequence():
    seq = synth.ba_sequence(200, 3000, 300)
    mask = synth.inject_outliers(seq, 0.03, (50.0, 300.0), seed=5)
    return seq, mask


def _weights_flag_the_outliers(w, seq, mask):
    cm = _constrained(seq, mask)
    assert cm.sum() >= 500
    assert np.quantile(w[cm], 0.99) < W_OUTLIER_P99 and np.quantile(w[~mask], 0.01) > W_INLIER_P01


def test_outlier_recovery(gpu):
    """~3 % gross mismatches on a 300-keyframe sweep: the Gaussian solve is dragged off the ground truth, Cauchy and
    Huber are not; Cauchy's final weights single out the injected outliers."""
    seq, mask = _recovery_sequence()
    out = {}
    for name, loss in (("gaussian", None), ("cauchy", LOSSES["cauchy"]), ("huber", LOSSES["huber"])):
        prob, sv = _problem(seq, loss)
        poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
        out[name] = (_rms_t(poses.cpu().numpy(), seq), sv.stereo_weights(poses, points).cpu().numpy() if loss else None,
                     rep.iterations)
    print("robust recovery: rms_t", {n: v[0] for n, v in out.items()}, "iterations", {n: v[2] for n, v in out.items()})
    assert out["gaussian"][0] > RMS_BOUND
    assert out["cauchy"][0] < RMS_BOUND and out["huber"][0] < RMS_BOUND
    _weights_flag_the_outliers(out["cauchy"][1], seq, mask)


def _robust_graph(seq, model):
    """batch.py:295-305's emission loop with a robust landmark noise model"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    n_kf, nL = len(seq["poses_gt"]), len(seq["points_gt"])
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(seq["poses_gt"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])))
    K = gtsam.Cal3_S2Stereo(*seq["K"])
    for i in range(n_kf):
        values.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
    for j in range(nL):
        values.insert(L(j), seq["points_init"][j])
    for a in range(len(seq["obs_pose"])):
        graph.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*seq["meas"][a]), model,
                                                    X(int(seq["obs_pose"][a])), L(int(seq["obs_point"][a])), K))
    return graph, values


def test_gtsam_drop_in_path(gpu, oracle):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    kind, k = LOSSES["cauchy"]
    seq, mask = _recovery_sequence()
    n_kf = len(seq["poses_gt"])
    noise = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Cauchy.Create(k),
                                           gtsam.noiseModel.Isotropic.Sigma(3, seq["sigma"]))
    graph, initial = _robust_graph(seq, noise)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    prob, sv = _problem(seq, (kind, k))
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    got = np.stack([result.atPose3(X(i)).flat12() for i in range(n_kf)])
    got_pts = np.stack([result.atPoint3(L(j)) for j in range(len(seq["points_gt"]))])
    assert opt.report().tries == rep.tries and opt.report().outer == rep.outer
    assert relerr(got, poses.cpu().numpy()) < 1e-9 and relerr(got_pts, points.cpu().numpy()) < 1e-8
    R = _ref(oracle, prob, seq, kind, k)
    assert graph.error(result) == pytest.approx(R.error(got, got_pts), rel=1e-11)
    assert opt.error() == pytest.approx(graph.error(result), rel=1e-9)
    pkeys, lkeys, w = opt.report().stereo_weights
    flag = {(int(p), int(q)): float(x) for p, q, x in zip(pkeys, lkeys, w)}
    assert len(flag) == len(w) == len(seq["meas"])
    wi = np.array([flag[(X(int(i)), L(int(j)))] for i, j in zip(seq["obs_pose"], seq["obs_point"])])
    assert np.abs(wi - sv.stereo_weights(poses, points).cpu().numpy()).max() < 1e-9
    _weights_flag_the_outliers(wi, seq, mask)
    # the Gaussian graph keeps no weights
    g2, i2 = _robust_graph(seq, gtsam.noiseModel.Isotropic.Sigma(3, seq["sigma"]))
    o2 = gtsam.LevenbergMarquardtOptimizer(g2, i2, gtsam.LevenbergMarquardtParams())
    o2.optimize()
    assert o2.report().stereo_weights is None


def _nav(oracle, seq, loss):
    from test_nav_oracle import build_nav
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavFactors
    n_kf = len(seq["poses_gt"])
    P, N = build_nav(oracle, seq, zero_velocity_prior=False)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, len(seq["points_gt"]), seq["K"],
                           seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None],
                           pose_stride=2, loss=loss)
    nav = NavFactors(seq["gravity"], imu=(N.imu_i, N.imu_j, N.imu_pim, N.imu_W),
                     dvl=(N.dvl_pose, N.dvl_meas, 1.0 / N.dvl_w), vprior=(N.vp_idx, N.vp_v, 1.0 / N.vp_w))
    sv = NavBASolver(prob, nav)
    return sv.optimize(d(seq["poses_init"]), d(np.zeros_like(seq["vels_gt"])), d(np.zeros(6)), d(seq["points_init"]))


def test_nav_graph_with_robust_stereo_factors(gpu, oracle):
    seq = synth.nav_sequence(16, 400, 80)
    g = _nav(oracle, seq, None)
    h = _nav(oracle, seq, ("huber", 1e12))
    assert (h[4].outer, h[4].tries) == (g[4].outer, g[4].tries)
    for a, b in zip(h[:4], g[:4]):
        assert relerr(a.cpu().numpy(), b.cpu().numpy()) <= 1e-10
    mask = synth.inject_outliers(seq, 0.03, (50.0, 300.0), seed=9)
    assert mask.sum() > 10
    rg = _rms_t(_nav(oracle, seq, None)[0].cpu().numpy(), seq)
    rc = _rms_t(_nav(oracle, seq, LOSSES["cauchy"])[0].cpu().numpy(), seq)
    print("nav robust recovery: rms_t gaussian %.4g cauchy %.4g" % (rg, rc))
    assert rg > NAV_RMS_BOUND > rc


def _sharded_robust_worker(rank, world, size=(60, 900, 150)):
    from visual_underwater_slam_amd import dist as vdist
    torch.cuda.set_device(0)
    seq = synth.ba_sequence(*size)
    synth.inject_outliers(seq, 0.05, (50.0, 300.0))
    nL = len(seq["points_gt"])
    sv = vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], size[0], nL, seq["K"], seq["sigma"],
                                     prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None],
                                     loss=LOSSES["cauchy"])
    poses, pts_local, rep = sv.optimize(torch.from_numpy(seq["poses_init"]).cuda(), torch.from_numpy(seq["points_init"]).cuda())
    pts = sv.gather_points(pts_local, nL)
    return poses.cpu().numpy(), pts.cpu().numpy(), rep.err_hist, rep.tries


def test_sharded_robust_lm_two_ranks_on_one_gpu_matches_single(gpu):
    from test_dist import _run
    out = _run(_sharded_robust_worker, 2)
    seq = synth.ba_sequence(60, 900, 150)
    synth.inject_outliers(seq, 0.05, (50.0, 300.0))
    prob, sv = _problem(seq, LOSSES["cauchy"])
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    for r in range(2):
        p, pt, hist, tries = out[r]
        assert tries == rep.tries and np.allclose(hist, rep.err_hist, rtol=1e-9)
        assert np.abs(p - poses.cpu().numpy()).max() < 1e-9 * max(1.0, np.abs(p).max())
        assert np.abs(pt - points.cpu().numpy()).max() < 1e-8 * np.abs(pt).max()
    assert np.array_equal(out[0][0], out[1][0])
