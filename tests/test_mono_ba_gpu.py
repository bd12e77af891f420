"""Monocular projection factors next to the stereo factors on the MI355X (include/vus_mono.h): the `_mixed` kernels stage
by stage against the numpy reference (tests/mono_ref.py) on the problem of tests/mono_problem.py, all flags 0 against
today's entry points, the dropped-row identity, the LM against the reference LM, the gtsam drop-in path with its
marginals, an inertial graph, and the sharded solver's refusal."""
import ctypes

import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
from conftest import same_lm_trajectory
import mono_problem
import mono_ref
import sensor_ref

pytestmark = pytest.mark.gpu

S = sensor_ref.extrinsic()
LOSSES = {"gaussian": (0, 0.0), "huber": (1, 1.345), "cauchy": (2, 2.3849)}
MONO_LM, STEREO_LM = mono_problem.MONO_LM, mono_problem.STEREO_LM


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(seq, loss, sensor, mono=True, **kw):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    if mono:
        kw.update(mono=seq["mono"], mono_K=seq["mono_K"], mono_sigma=seq["mono_sigma"])
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], len(seq["poses_gt"]), len(seq["points_gt"]),
                           seq["K"], seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1],
                           prior_sigmas=seq["prior_sigmas"][None], loss=loss if loss and loss[0] else None,
                           body_P_sensor=sensor, **kw)
    return prob, StereoBASolver(prob)


def _ref(oracle, prob, seq, kind, k, sensor, cls=mono_ref.MonoBA):
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    perm = pk["perm"].numpy().astype(np.int64)
    return cls(oracle, pk, seq["K"], seq["sigma"], kind, k, sensor, np.asarray(seq["mono"])[perm], seq["mono_K"],
               seq["mono_sigma"], (np.array([0]), seq["poses_gt"][:1], seq["prior_sigmas"][None]))


def _stage_sequence(sensor, **kw):
    """5 % outliers; landmark STEREO_LM (stereo sightings only) and landmark MONO_LM (mono sightings only) behind every
    camera that sees them; with an extrinsic the poses are the body poses X = C o S^-1"""
    seq = mono_problem.mixed_sequence(outliers=0.05, **kw)
    seq["points_init"] = seq["points_init"].copy()
    seq["points_init"][STEREO_LM, 2] = -1.0
    seq["points_init"][MONO_LM, 2] = -1.5
    return seq if sensor is None else sensor_ref.body_sequence(seq, sensor)


def _compare_stages(sv, prob, R, seq, tag):
    """linearize, both errors, one schur -> band_solve -> backsub -> eval_step trial and the weights against R"""
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv.linearize(poses, points)
    lin = R.linearize(seq["poses_init"], seq["points_init"])
    got = {"W": sv.W, "V": sv.V, "gl": sv.gl, "Hpp": sv.Hpp, "gp": sv.gp}
    errs = {key: relerr(v.cpu().numpy(), lin[key]) for key, v in got.items()}
    print(f"mono stages {tag}: {errs}")
    for key, v in got.items():
        assert torch.isfinite(v).all(), key
    for key, e in errs.items():
        assert e <= 1e-11, key
    assert float(sv.scal[0]) == pytest.approx(lin["err"], rel=1e-11)
    assert sv.error(poses, points) == pytest.approx(R.error(seq["poses_init"], seq["points_init"]), rel=1e-11)
    sv.schur(1e-3); sv.band_solve(); sv.backsub()
    sv.eval_step(poses, points)
    dp, dl = sv.dp.cpu().numpy(), sv.dl.cpu().numpy()
    npo, npt, lin1, new1 = R.eval_step(seq["poses_init"], seq["points_init"], dp, dl)
    print(f"mono stages {tag}: linear {float(sv.scal[1])!r} vs {lin1!r}, new {float(sv.scal[2])!r} vs {new1!r}")
    assert float(sv.scal[1]) == pytest.approx(lin1, rel=1e-11)
    assert float(sv.scal[2]) == pytest.approx(new1, rel=1e-11)
    assert lin1 < lin["err"]
    assert relerr(sv.new_poses.cpu().numpy(), npo) <= 1e-12
    assert relerr(sv.new_points.cpu().numpy(), npt) <= 1e-12
    perm = prob.pk["perm"].cpu().numpy().astype(np.int64)
    w = sv.stereo_weights(poses, points).cpu().numpy()
    want = np.empty_like(w)
    want[perm] = lin["w"]
    assert w.shape == (len(seq["obs_pose"]),) and np.abs(w - want).max() <= 1e-11
    return lin, w


@pytest.mark.parametrize("with_sensor", (False, True))
@pytest.mark.parametrize("name", ("gaussian", "huber", "cauchy"))
def test_mixed_stages_match_the_reference(gpu, oracle, name, with_sensor):
    kind, k = LOSSES[name]
    sensor = S if with_sensor else None
    seq = _stage_sequence(sensor)
    mono_problem.check_topology(seq)
    prob, sv = _problem(seq, (kind, k), sensor)
    assert prob.has_mono and prob.has_sensor == with_sensor and prob.robust == (kind != 0)
    assert sv._loss_args("vus_ba_linearize")[0] == "vus_ba_linearize_mixed"
    R = _ref(oracle, prob, seq, kind, k, sensor)
    lin, w = _compare_stages(sv, prob, R, seq, f"{name} sensor={with_sensor}")
    # cheirality, judged in the camera frame, for each kind: zero Jacobian rows here and in the reference
    ol = prob.pk["obs_point"].cpu().numpy()
    for lm in (STEREO_LM, MONO_LM):
        sel = ol == lm
        assert sel.any() and not sv.W.cpu().numpy()[sel].any() and not lin["W"][sel].any()
        if kind:
            assert np.all(w[seq["obs_point"] == lm] < 1.0)
    if kind == 0:
        assert np.all(w == 1.0) and np.abs(lin["W"][~np.isin(ol, (STEREO_LM, MONO_LM))]).max(1).min() > 0
    else:
        assert (w[seq["mono"]] < 1.0).any() and (w[~seq["mono"]] < 1.0).any()


def _force_mixed(prob, mono_K, mono_sigma):
    """route a problem WITHOUT mono observations through the `_mixed` entry points, every flag 0"""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import _CMono
    prob.is_mono_L = torch.zeros(prob.n_obs, dtype=torch.uint8, device=prob.device)
    prob.c_mono = _CMono(_lib.ptr(prob.is_mono_L), (ctypes.c_double * 5)(*mono_K), 1.0 / mono_sigma)
    prob.has_mono = True


@pytest.mark.parametrize("with_sensor", (False, True))
@pytest.mark.parametrize("name", ("gaussian", "huber"))
def test_all_flags_zero_equals_todays_entry_points(gpu, name, with_sensor):
    """vus_ba_*_mixed with is_mono = 0 everywhere against vus_ba_* / `_robust` / `_sensor` on the same problem"""
    sensor = S if with_sensor else None
    seq = _stage_sequence(sensor, mono_frac=0.0)
    assert not seq["mono"].any() and np.isfinite(seq["meas"]).all()
    loss = LOSSES[name]
    prob_m, sv_m = _problem(seq, loss, sensor, mono=False)
    prob_0, sv_0 = _problem(seq, loss, sensor, mono=False)
    _force_mixed(prob_m, seq["mono_K"], seq["mono_sigma"])
    today = {(False, False): "vus_ba_linearize", (True, False): "vus_ba_linearize_robust"}.get((loss[0] != 0, with_sensor),
                                                                                             "vus_ba_linearize_sensor")
    assert sv_m._loss_args("vus_ba_linearize")[0] == "vus_ba_linearize_mixed" and sv_0._loss_args("vus_ba_linearize")[0] == today
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv_m.linearize(poses, points)
    sv_0.linearize(poses, points)
    pairs = {"W": (sv_m.W, sv_0.W), "V": (sv_m.V, sv_0.V), "gl": (sv_m.gl, sv_0.gl), "Hpp": (sv_m.Hpp, sv_0.Hpp),
             "gp": (sv_m.gp, sv_0.gp), "err": (sv_m.scal[:1], sv_0.scal[:1])}
    errs = {key: relerr(a.cpu().numpy(), b.cpu().numpy()) for key, (a, b) in pairs.items()}
    print(f"all flags 0 {name} sensor={with_sensor}: {errs}")
    for key, e in errs.items():
        assert e <= 1e-14, key
    assert sv_m.error(poses, points) == pytest.approx(sv_0.error(poses, points), rel=1e-14)
    for sv in (sv_m, sv_0):
        sv.schur(1e-3); sv.band_solve(); sv.backsub()
    sv_m.dp.copy_(sv_0.dp); sv_m.dl.copy_(sv_0.dl)          # the same step into both step evaluations
    sv_m.eval_step(poses, points)
    sv_0.eval_step(poses, points)
    assert relerr(sv_m.scal[1:3].cpu().numpy(), sv_0.scal[1:3].cpu().numpy()) <= 1e-14
    assert relerr(sv_m.new_poses.cpu().numpy(), sv_0.new_poses.cpu().numpy()) <= 1e-14
    assert relerr(sv_m.stereo_weights(poses, points).cpu().numpy(), sv_0.stereo_weights(poses, points).cpu().numpy()) <= 1e-14


class _DroppedRow(mono_ref.MonoBA):
    """the all-stereo factors with their uR rows deleted"""

    def factors(self, poses, points, jac=True):
        r, H1, H2 = super().factors(poses, points, jac)
        r[:, 1], H1[:, 1], H2[:, 1] = 0.0, 0.0, 0.0
        return r, H1, H2


def test_all_mono_graph_is_the_stereo_graph_without_its_uR_rows(gpu, oracle):
    """every observation mono with K_mono = (fx, fy, 0, cx, cy) and sigma_mono = sigma: against MonoBA, and against the
    all-stereo graph's reference with the uR rows deleted -- the identity holds in the reference, not only in the kernel"""
    st = _stage_sequence(None, mono_frac=0.0)
    K = st["K"]
    mo = dict(st)
    mo["mono"] = np.ones(len(st["meas"]), bool)
    mo["mono_K"], mo["mono_sigma"] = np.array([K[0], K[1], 0.0, K[3], K[4]]), st["sigma"]
    mo["meas"] = st["meas"].copy()
    mo["meas"][:, 1] = np.nan
    st["mono_K"], st["mono_sigma"] = mo["mono_K"], mo["mono_sigma"]
    prob, sv = _problem(mo, None, None)
    R_mono = _ref(oracle, prob, mo, 0, 0.0, None)
    R_drop = _ref(oracle, prob, st, 0, 0.0, None, cls=_DroppedRow)
    R_drop.meas = np.ascontiguousarray(st["meas"][prob.pk["perm"].cpu().numpy().astype(np.int64)])
    assert R_mono.is_mono.all() and not R_drop.is_mono.any()
    _compare_stages(sv, prob, R_mono, mo, "all mono")
    a, b = R_mono.linearize(mo["poses_init"], mo["points_init"]), R_drop.linearize(st["poses_init"], st["points_init"])
    sv.linearize(d(mo["poses_init"]), d(mo["points_init"]))
    for key, v in {"W": sv.W, "V": sv.V, "gl": sv.gl, "Hpp": sv.Hpp, "gp": sv.gp}.items():
        assert relerr(a[key], b[key]) <= 1e-12, key               # reference against reference: the identity itself
        assert relerr(v.cpu().numpy(), b[key]) <= 1e-11, key
    assert a["err"] == pytest.approx(b["err"], rel=1e-12) and float(sv.scal[0]) == pytest.approx(b["err"], rel=1e-11)


# -- LM and the drop-in path: a smaller draw of the same generator (16 keyframes, 80 landmarks, keyframe 3 sees all) -------
def _lm_sequence(sensor, outliers):
    """gross outliers only where a robust model meets them (under the Gaussian model they make LM reject most trials on
    decisions a rounding error can turn)"""
    seq = mono_problem.mixed_sequence(n_kf=16, n_lm=80, outliers=outliers)
    assert seq["mono"][seq["obs_point"] == MONO_LM].all() and (seq["obs_point"] == MONO_LM).sum() >= 2
    assert 0.3 < seq["mono"].mean() < 0.5
    return seq if sensor is None else sensor_ref.body_sequence(seq, sensor)


_lm_cache = {}


def _reference_lm(oracle, prob, seq, name, sensor):
    """the reference LM of one case, computed once and shared (read only)"""
    key = (name, sensor is not None)
    if key not in _lm_cache:
        _lm_cache[key] = _ref(oracle, prob, seq, *LOSSES[name], sensor).lm(seq["poses_init"], seq["points_init"])
    return _lm_cache[key]


@pytest.mark.parametrize("name,with_sensor", (("gaussian", False), ("cauchy", True)))
def test_mixed_lm_walks_the_reference_lm(gpu, oracle, name, with_sensor):
    sensor = S if with_sensor else None
    seq = _lm_sequence(sensor, 0.10 if LOSSES[name][0] else 0.0)
    prob, sv = _problem(seq, LOSSES[name], sensor)
    rposes, rpoints, rrep = _reference_lm(oracle, prob, seq, name, sensor)
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    assert rrep["outer"] >= 3
    print(f"mono LM {name}: outer {rep.outer} tries {rep.tries} error {rep.initial_error:.6g} -> {rep.final_error:.6g}; "
          f"lambda {rep.lambda_hist} vs {rrep['lambda_hist']}")
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    e_pose, e_pt = relerr(poses.cpu().numpy(), rposes), relerr(points.cpu().numpy(), rpoints)
    print(f"mono LM {name}: poses vs reference {e_pose:.2g}, points {e_pt:.2g}")
    assert e_pose <= 1e-6 and e_pt <= 1e-6          # the bound err_hist holds
    assert rep.final_error < rep.initial_error


def _shim_graph(seq, noise3, noise2, sensor, as_block):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(seq["poses_gt"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])))
    K3, K2 = gtsam.Cal3_S2Stereo(*seq["K"]), gtsam.Cal3_S2(*seq["mono_K"])
    Sp = gtsam.Pose3.from_flat12(sensor)
    for i in range(len(seq["poses_gt"])):
        values.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
    for j in range(len(seq["points_gt"])):
        values.insert(L(j), seq["points_init"][j])
    mono, meas = seq["mono"], seq["meas"]
    pk, lk = X(0) + seq["obs_pose"].astype(np.int64), L(0) + seq["obs_point"].astype(np.int64)
    if as_block:
        graph.push_back(gtsam.StereoFactorBlock(meas[~mono], noise3, pk[~mono], lk[~mono], K3, Sp))
        graph.push_back(gtsam.ProjectionFactorBlock(meas[mono][:, [0, 2]], noise2, pk[mono], lk[mono], K2, Sp))
    else:
        for a in range(len(meas)):
            if mono[a]:
                graph.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(meas[a, 0], meas[a, 2]), noise2,
                                                                     int(pk[a]), int(lk[a]), K2, Sp))
            else:
                graph.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*meas[a]), noise3, int(pk[a]), int(lk[a]), K3, Sp))
    return graph, values


@pytest.mark.parametrize("as_block", (False, True))
def test_gtsam_drop_in_path_with_both_kinds_of_factor(gpu, oracle, as_block):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    name = "cauchy"
    kind, k = LOSSES[name]
    seq = _lm_sequence(S, 0.10)
    est = gtsam.noiseModel.mEstimator.Cauchy.Create(k)
    noise3 = gtsam.noiseModel.Robust.Create(est, gtsam.noiseModel.Isotropic.Sigma(3, seq["sigma"]))
    noise2 = gtsam.noiseModel.Robust.Create(est, gtsam.noiseModel.Isotropic.Sigma(2, seq["mono_sigma"]))
    graph, initial = _shim_graph(seq, noise3, noise2, S, as_block)
    assert graph.nrFactors() == len(seq["meas"]) + 1
    prob, sv = _problem(seq, (kind, k), S)
    R = _ref(oracle, prob, seq, kind, k, S)
    assert graph.error(initial) == pytest.approx(R.error(seq["poses_init"], seq["points_init"]), rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rposes, rpoints, rrep = _reference_lm(oracle, prob, seq, name, S)
    rep = opt.report()
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    assert len(rep.stereo_weights[2]) == len(seq["meas"])        # a weight for every observation, mono included
    poses, points, _ = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    got = np.stack([result.atPose3(X(i)).flat12() for i in range(len(seq["poses_gt"]))])
    got_pts = np.stack([result.atPoint3(L(j)) for j in range(len(seq["points_gt"]))])
    assert relerr(got, poses.cpu().numpy()) < 1e-9 and relerr(got_pts, points.cpu().numpy()) < 1e-8
    # marginals of one pose and of the mono-only landmark: the shim against the array path, the array path against the
    # dense inverse of the reference's Hessian
    mg = gtsam.Marginals(graph, result)
    m = sv.marginals(poses, points)
    assert relerr(mg.marginalCovariance(X(3)), m.pose_cov[3].cpu().numpy()) < 1e-8
    assert relerr(mg.marginalCovariance(L(MONO_LM)), m.point_cov[MONO_LM].cpu().numpy()) < 1e-8
    nP = len(seq["poses_gt"])
    Hinv = np.linalg.inv(R.full_hessian(poses.cpu().numpy(), points.cpu().numpy()))
    at = 6 * nP + 3 * MONO_LM
    e_pose = relerr(m.pose_cov[3].cpu().numpy(), Hinv[18:24, 18:24])
    e_lm = relerr(m.point_cov[MONO_LM].cpu().numpy(), Hinv[at:at + 3, at:at + 3])
    print(f"mono marginals: pose 3 {e_pose:.2g}, mono-only landmark {e_lm:.2g}")
    assert e_pose < 1e-9 and e_lm < 1e-9


def test_a_graph_of_mono_factors_only_optimizes(gpu, oracle):
    """the shim accepts a graph whose landmark factors are all monocular (the gauge: priors on two poses, which fix the
    scale); its error and its LM are the reference's"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    seq = mono_problem.mixed_sequence(mono_frac=1.0, n_kf=16, n_lm=80)
    assert seq["mono"].all()
    graph, initial = gtsam.NonlinearFactorGraph(), gtsam.Values()
    prior = gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])
    for i in (0, 15):
        graph.add(gtsam.PriorFactorPose3(X(i), gtsam.Pose3.from_flat12(seq["poses_gt"][i]), prior))
    for i in range(16):
        initial.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
    for j in range(80):
        initial.insert(L(j), seq["points_init"][j])
    graph.push_back(gtsam.ProjectionFactorBlock(seq["meas"][:, [0, 2]], gtsam.noiseModel.Isotropic.Sigma(2, seq["mono_sigma"]),
                                                X(0) + seq["obs_pose"].astype(np.int64), L(0) + seq["obs_point"].astype(np.int64),
                                                gtsam.Cal3_S2(*seq["mono_K"])))
    from visual_underwater_slam_amd.ba import StereoBAProblem
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], 16, 80, seq["K"], seq["sigma"], mono=seq["mono"],
                           mono_K=seq["mono_K"], mono_sigma=seq["mono_sigma"])
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    R = mono_ref.MonoBA(oracle, pk, seq["K"], seq["sigma"], 0, 0.0, None, np.ones(len(seq["meas"]), bool), seq["mono_K"],
                        seq["mono_sigma"], (np.array([0, 15]), seq["poses_gt"][[0, 15]], np.tile(seq["prior_sigmas"], (2, 1))))
    e0 = R.error(seq["poses_init"], seq["points_init"])
    assert graph.error(initial) == pytest.approx(e0, rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rep = opt.report()
    _, _, rrep = R.lm(seq["poses_init"], seq["points_init"])
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    assert rep.final_error < 0.1 * e0 and result.atPoint3(L(MONO_LM)).shape == (3,)


def test_inertial_graph_takes_the_mixed_route(gpu, oracle):
    """NavBASolver on a problem with mono observations: its stereo-side arrays after linearize() are the plain
    StereoBASolver's on the same problem, and differ from the all-stereo problem's"""
    from test_nav_oracle import build_nav
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver, NavBASolver, NavFactors
    seq = synth.nav_sequence(10, 200, 50)
    n_kf, nL, n = len(seq["poses_gt"]), len(seq["points_gt"]), len(seq["meas"])
    mono = synth._hash_uniform(np.arange(n, dtype=np.int64), mono_problem.SEED ^ 0x0F0F) < 0.4
    meas = seq["meas"].copy()
    meas[mono, 1] = np.nan
    K = seq["K"]
    mk = dict(mono=mono, mono_K=np.array([K[0], K[1], 0.7, K[3], K[4]]), mono_sigma=6.0)
    _, N = build_nav(oracle, seq, zero_velocity_prior=False)
    nav = NavFactors(seq["gravity"], imu=(N.imu_i, N.imu_j, N.imu_pim, N.imu_W),
                     dvl=(N.dvl_pose, N.dvl_meas, 1.0 / N.dvl_w), vprior=(N.vp_idx, N.vp_v, 1.0 / N.vp_w))
    common = dict(prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None])
    args = (seq["obs_pose"], seq["obs_point"], meas, n_kf, nL, K, seq["sigma"])
    nav_sv = NavBASolver(StereoBAProblem(*args, pose_stride=2, **common, **mk), nav)
    plain = StereoBASolver(StereoBAProblem(*args, **common, **mk))
    stereo_only = StereoBASolver(StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, nL, K, seq["sigma"], **common))
    assert nav_sv._loss_args("vus_ba_eval_step")[0] == "vus_ba_eval_step_mixed"
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    for sv in (nav_sv, plain, stereo_only):
        sv.linearize(poses, points)
    for key in ("W", "V", "gl", "Hpp", "gp"):
        a, b, c = (getattr(sv, key).cpu().numpy() for sv in (nav_sv, plain, stereo_only))
        assert np.isfinite(a).all() and np.array_equal(a, b), key
        assert relerr(a, c) > 1e-3, key
    assert nav_sv.error(poses, points) == plain.error(poses, points)
    out = nav_sv.optimize(poses, d(np.zeros_like(seq["vels_gt"])), d(np.zeros(6)), points)
    assert out[4].status == 0 and np.isfinite(out[4].final_error) and out[4].final_error < out[4].initial_error


def test_sharded_solver_refuses_a_problem_with_mono_observations(gpu):
    from visual_underwater_slam_amd import dist as vdist
    seq = mono_problem.mixed_sequence(n_kf=6, n_lm=20)
    with pytest.raises(NotImplementedError, match="mono"):
        vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, 20, seq["K"], seq["sigma"],
                                    mono=seq["mono"])
    prob, _ = _problem(seq, None, None)
    with pytest.raises(NotImplementedError, match="mono"):
        vdist._ShardSolver(prob, 1)


def test_the_library_validates_the_mono_descriptor(gpu):
    """bad K / sigma are refused by the C entry point with the library's negative status, before any launch"""
    from visual_underwater_slam_amd import _lib
    seq = mono_problem.mixed_sequence(n_kf=6, n_lm=20)
    prob, sv = _problem(seq, None, None)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    good = (tuple(seq["mono_K"]), 1.0 / seq["mono_sigma"])
    for K5, w, word in (((np.nan,) + good[0][1:], good[1], "finite"), ((-1.0,) + good[0][1:], good[1], "fx"),
                        (good[0], 0.0, "inv_sigma"), (good[0], np.inf, "inv_sigma")):
        prob.c_mono.K = (ctypes.c_double * 5)(*K5)
        prob.c_mono.inv_sigma = w
        with pytest.raises(_lib.VusError, match=word):
            sv.linearize(poses, points)
    prob.c_mono.K, prob.c_mono.inv_sigma = (ctypes.c_double * 5)(*good[0]), good[1]
    sv.linearize(poses, points)
    assert torch.isfinite(sv.W).all()
