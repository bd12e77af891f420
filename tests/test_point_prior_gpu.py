"""PriorFactorPoint3 on observed landmarks on the MI355X (include/vus_point_prior.h, ba.PointPriors, the solver hooks,
the gtsam shim) against the numpy reference tests/point_prior_ref.py on the problem of tests/mono_problem.py: the three
entry points stage by stage, the no-op and determinism guarantees, the LM, the drop-in path, the scale of a monocular
graph, the marginals of a landmark with a single mono sighting, an inertial graph and the refusals."""
import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
from conftest import same_lm_trajectory
import mono_problem
import mono_ref
import point_prior_ref as ppr
import sensor_ref

pytestmark = pytest.mark.gpu

S = sensor_ref.extrinsic()
LOSSES = {"gaussian": (0, 0.0), "cauchy": (2, 2.3849)}
STEREO_LM, MONO_LM, TRIPLE_LM, FAR_LM = ppr.STEREO_LM, ppr.MONO_LM, ppr.TRIPLE_LM, ppr.FAR_LM


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _point_priors(priors, n_points):
    from visual_underwater_slam_amd.ba import PointPriors
    return None if priors is None else PointPriors(*priors, n_points)


def _problem(seq, loss, sensor, priors=None):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], len(seq["poses_gt"]), len(seq["points_gt"]),
                           seq["K"], seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1],
                           prior_sigmas=seq["prior_sigmas"][None], loss=loss if loss and loss[0] else None,
                           body_P_sensor=sensor, mono=seq["mono"], mono_K=seq["mono_K"], mono_sigma=seq["mono_sigma"])
    return prob, StereoBASolver(prob, point_priors=_point_priors(priors, len(seq["points_gt"])))


def _ref(oracle, prob, seq, kind, k, sensor, priors, pose_priors=(0,)):
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    perm = pk["perm"].numpy().astype(np.int64)
    pp = np.array(pose_priors)
    return ppr.PointPriorBA(oracle, pk, seq["K"], seq["sigma"], kind, k, sensor, np.asarray(seq["mono"])[perm], seq["mono_K"],
                            seq["mono_sigma"], (pp, seq["poses_gt"][pp], np.tile(seq["prior_sigmas"], (len(pp), 1))),
                            point_priors=priors)


def _stage_sequence(sensor):
    """the default problem (70 keyframes, 310 landmarks) with 5 % outliers, one landmark cut down to a single mono
    sighting, and STEREO_LM (stereo sightings only, carries a prior) behind every camera that sees it; with an extrinsic
    the poses are the body poses X = C o S^-1"""
    seq, single_lm = ppr.single_sighting(mono_problem.mixed_sequence(outliers=0.05))
    seq["points_init"] = seq["points_init"].copy()
    seq["points_init"][STEREO_LM, 2] = -1.0
    return (seq if sensor is None else sensor_ref.body_sequence(seq, sensor)), single_lm


@pytest.mark.parametrize("with_sensor", (False, True))
@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_stages_match_the_reference(gpu, oracle, name, with_sensor):
    """vus_point_prior_linearize / _eval_step / _error after the `_mixed` calls: V, gl and the scalars at the tolerances
    of test_mono_ba_gpu.py::test_mixed_stages_match_the_reference (1e-11 relative)"""
    kind, k = LOSSES[name]
    sensor = S if with_sensor else None
    seq, single_lm = _stage_sequence(sensor)
    priors = ppr.prior_set(seq, single_lm)
    nL = len(seq["points_gt"])
    assert {0, nL - 1, single_lm, STEREO_LM, FAR_LM} <= set(priors[0].tolist()) and (priors[0] == TRIPLE_LM).sum() == 3
    assert np.abs(priors[1][priors[0] == FAR_LM] - seq["points_init"][FAR_LM]).max() > 3.0
    prob, sv = _problem(seq, (kind, k), sensor, priors)
    assert sv._loss_args("vus_ba_linearize")[0] == "vus_ba_linearize_mixed" and sv.Q.n == 8 and sv.Q.n_rows == 6
    R = _ref(oracle, prob, seq, kind, k, sensor, priors)
    p0, x0 = seq["poses_init"], seq["points_init"]
    poses, points = d(p0), d(x0)
    sv.linearize(poses, points)
    V0, gl0, obs0 = sv.V.cpu().numpy().copy(), sv.gl.cpu().numpy().copy(), float(sv.scal[0])
    sv.point_prior_linearize(points)
    lin = R.linearize(p0, x0)
    V, gl = sv.V.cpu().numpy(), sv.gl.cpu().numpy()
    errs = {"V": relerr(V, lin["V"]), "gl": relerr(gl, lin["gl"])}
    print(f"point prior stages {name} sensor={with_sensor}: {errs}; scalars {obs0!r} vs {lin['obs_err']!r}, "
          f"{float(sv.pp_scal[0])!r} vs {lin['pp_err']!r}")
    assert np.isfinite(V).all() and np.isfinite(gl).all()
    assert errs["V"] <= 1e-11 and errs["gl"] <= 1e-11
    # the prior's scalar has a slot of its own: the observations' scalar is untouched
    assert float(sv.scal[0]) == obs0 and obs0 == pytest.approx(lin["obs_err"], rel=1e-11)
    assert float(sv.pp_scal[0]) == pytest.approx(lin["pp_err"], rel=1e-11)
    # only the xx / yy / zz slots of prior-carrying landmarks moved, and by sum w^2 whatever the robust model is
    carrying = np.unique(priors[0])
    dV, dg = V - V0, gl - gl0
    rest = np.setdiff1d(np.arange(nL), carrying)
    assert not dV[rest].any() and not dg[rest].any() and not dV[:, [1, 2, 4]].any()
    Vp, glp = R.prior_blocks(x0)
    assert relerr(dV[carrying], Vp[carrying]) <= 1e-11 and relerr(dg[carrying], glp[carrying]) <= 1e-11
    # the landmark behind its cameras: no information from its observations, the prior's alone is left
    ol = prob.pk["obs_point"].cpu().numpy()
    assert not sv.W.cpu().numpy()[ol == STEREO_LM].any() and not V0[STEREO_LM].any()
    assert np.array_equal(V[STEREO_LM, [0, 3, 5]], np.full(3, 100.0)) or relerr(V[STEREO_LM, [0, 3, 5]], np.full(3, 100.0)) <= 1e-14
    # the landmark with one mono sighting: rank 2 without the prior, full rank with it
    sym = lambda v: np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]])
    assert np.linalg.matrix_rank(sym(V0[single_lm]), tol=1e-9 * np.abs(V0[single_lm]).max()) == 2
    assert np.linalg.eigvalsh(sym(V[single_lm])).min() > 1.0
    # one trial: schur -> band solve -> back-substitution -> both step evaluations
    sv.schur(1e-3); sv.band_solve(); sv.backsub()
    sv.eval_step(poses, points)
    sv.point_prior_eval_step(points)
    dp, dl = sv.dp.cpu().numpy(), sv.dl.cpu().numpy()
    lin1, new1 = R.observation_errors(p0, x0, dp, dl)
    npo, npt = R.retract(p0, x0, dp, dl)
    pp1, pp2 = R.prior_error(x0 + dl), R.prior_error(npt)
    got = [float(x) for x in sv.pp_scal.cpu()]
    print(f"point prior stages {name}: linear {float(sv.scal[1])!r} vs {lin1!r}, new {float(sv.scal[2])!r} vs {new1!r}; "
          f"prior {got[1]!r} vs {pp1!r}, {got[2]!r} vs {pp2!r}")
    assert float(sv.scal[1]) == pytest.approx(lin1, rel=1e-11) and float(sv.scal[2]) == pytest.approx(new1, rel=1e-11)
    assert got[1] == pytest.approx(pp1, rel=1e-11) and got[2] == pytest.approx(pp2, rel=1e-11)
    assert got[1] == pytest.approx(got[2], rel=1e-12)            # the factor is linear: the two differ by round-off
    assert relerr(sv.new_points.cpu().numpy(), npt) <= 1e-12
    assert lin1 + pp1 < lin["err"]
    # the whole record is what one blocking read delivers
    status, sc = sv._lm_eval((poses, points))
    assert status == 0 and sc[1] == pytest.approx(lin1 + pp1, rel=1e-11) and sc[2] == pytest.approx(new1 + pp2, rel=1e-11)
    assert sc[0] == pytest.approx(lin["err"], rel=1e-11)
    # the two errors (last: error() reuses the record's first slot)
    assert sv.error(poses, points) == pytest.approx(mono_ref.MonoBA.error(R, p0, x0), rel=1e-11)
    assert sv.point_prior_error(points) == pytest.approx(R.prior_error(x0), rel=1e-11)
    assert sv._lm_error((poses, points)) == pytest.approx(R.error(p0, x0), rel=1e-11)


def _raw_calls(Q, points, dl, new_points, V, gl):
    """the three entry points called directly on copies of V / gl: (V, gl, err, out[2], error) as numpy"""
    from visual_underwater_slam_amd import _lib
    p, st = _lib.ptr, _lib.current_stream_ptr()
    V, gl = V.clone(), gl.clone()
    scal = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.empty((int(_lib.load().vus_point_prior_work_doubles(Q.addr())),), dtype=torch.float64, device="cuda")
    _lib.call("vus_point_prior_linearize", Q.addr(), p(points), p(V), p(gl), p(scal), p(work), st)
    _lib.call("vus_point_prior_eval_step", Q.addr(), p(points), p(dl), p(new_points), p(scal[1:]), p(work), st)
    _lib.call("vus_point_prior_error", Q.addr(), p(points), p(scal[3:]), p(work), st)
    return V.cpu().numpy(), gl.cpu().numpy(), scal.cpu().numpy()


@pytest.mark.parametrize("rows", (256, 257, 310))
def test_many_rows_cross_the_workgroup_boundary_and_two_runs_are_bit_identical(gpu, rows):
    """256, 257 or 310 prior-carrying landmarks (exactly one workgroup of 256 rows; a second one with a single live row;
    more than one and no multiple of it) plus the adversarial set, on arbitrary V / gl: the increments and the three
    scalars against the reference's prior term, and every output of two calls on the same inputs bit for bit"""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import PointPriors
    seq, single_lm = ppr.single_sighting(mono_problem.mixed_sequence(n_lm=rows))
    nL = len(seq["points_gt"])
    U = synth._hash_uniform
    a = np.arange(3 * nL, dtype=np.int64)
    idx0, mean0, sig0 = ppr.prior_set(seq, single_lm)
    every = np.arange(nL)[::-1]                                            # descending: the sort has work to do
    idx = np.concatenate([idx0[:4], every, idx0[4:]])
    mean = np.concatenate([mean0[:4], seq["points_gt"][every] + U(a, 11).reshape(nL, 3) - 0.5, mean0[4:]])
    sig = np.concatenate([sig0[:4], 0.05 + 3.0 * U(a, 12).reshape(nL, 3), sig0[4:]])
    Q = PointPriors(idx, mean, sig, nL)
    assert (Q.n, Q.n_rows) == (nL + 8, nL) and nL == rows
    _lib.call("vus_point_prior_check", Q.addr(), _lib.current_stream_ptr())
    assert int(_lib.load().vus_point_prior_work_doubles(Q.addr())) >= 4
    pk = {"n_poses": len(seq["poses_gt"]), "n_points": nL, "n_obs": len(seq["meas"]), "obs_pose": seq["obs_pose"],
          "obs_point": seq["obs_point"], "meas": seq["meas"]}
    R = ppr.PointPriorBA(None, pk, seq["K"], seq["sigma"], 0, 0.0, None, seq["mono"], seq["mono_K"], seq["mono_sigma"],
                         point_priors=(idx, mean, sig))
    x0 = seq["points_init"]
    dl = 0.2 * (U(a, 13).reshape(nL, 3) - 0.5)
    V0, gl0 = 50.0 * U(np.arange(6 * nL, dtype=np.int64), 14).reshape(nL, 6), 10.0 * (U(a, 15).reshape(nL, 3) - 0.5)
    args = (Q, d(x0), d(dl), d(x0 + dl), d(V0), d(gl0))
    V, gl, scal = _raw_calls(*args)
    Vp, glp = R.prior_blocks(x0)
    assert relerr(V - V0, Vp) <= 1e-11 and relerr(gl - gl0, glp) <= 1e-11 and not (V - V0)[:, [1, 2, 4]].any()
    want = [R.prior_error(x0), R.prior_error(x0 + dl), R.prior_error(x0 + dl), R.prior_error(x0)]
    print(f"point priors, {Q.n_rows} rows: scalars {scal.tolist()} vs {want}")
    assert np.allclose(scal, want, rtol=1e-11, atol=0)
    assert scal[1] == pytest.approx(scal[2], rel=1e-14) and scal[0] == pytest.approx(scal[3], rel=1e-14)
    V2, gl2, scal2 = _raw_calls(*args)
    assert np.array_equal(V, V2) and np.array_equal(gl, gl2) and np.array_equal(scal, scal2)


def _lm_sequence(sensor, outliers):
    """the smaller draw of test_mono_ba_gpu.py (16 keyframes, 80 landmarks), one landmark cut down to one mono sighting"""
    seq, single_lm = ppr.single_sighting(mono_problem.mixed_sequence(n_kf=16, n_lm=80, outliers=outliers))
    return (seq if sensor is None else sensor_ref.body_sequence(seq, sensor)), single_lm


LM_CASES = {"gaussian": (None, 0.0), "cauchy": (S, 0.10)}
_lm_cache = {}


def _lm_case(oracle, name):
    """problem, solver with priors, reference and the reference LM of one case, computed once and shared (read only)"""
    if name not in _lm_cache:
        sensor, outliers = LM_CASES[name]
        seq, single_lm = _lm_sequence(sensor, outliers)
        priors = ppr.prior_set(seq, single_lm)
        prob, sv = _problem(seq, LOSSES[name], sensor, priors)
        R = _ref(oracle, prob, seq, *LOSSES[name], sensor, priors)
        _lm_cache[name] = dict(seq=seq, single_lm=single_lm, priors=priors, prob=prob, sv=sv, R=R, sensor=sensor,
                               lm=R.lm(seq["poses_init"], seq["points_init"]))
    return _lm_cache[name]


def test_no_priors_is_a_no_op(gpu):
    """n == 0 at the C ABI (sums 0, V / gl untouched, nothing else written) and point_priors=None / an empty PointPriors
    in the solver: stages and a whole optimize() bit-identical to the solver built without the argument.  16 keyframes are
    two 8-pose panels: every row of the band solve's back-substitution then has a single contribution, so the LM is
    reproducible bit for bit and the comparison is exact."""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import PointPriors, StereoBASolver
    seq, _ = _lm_sequence(None, 0.0)
    nL = len(seq["points_gt"])
    empty = PointPriors([], np.zeros((0, 3)), np.zeros((0, 3)), nL)
    _lib.call("vus_point_prior_check", empty.addr(), _lib.current_stream_ptr())
    prob, plain = _problem(seq, None, None)
    plain = StereoBASolver(prob)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    plain.linearize(poses, points)
    V0, gl0 = plain.V.cpu().numpy().copy(), plain.gl.cpu().numpy().copy()
    V, gl, scal = _raw_calls(empty, points, plain.dl.zero_(), points, plain.V, plain.gl)
    assert np.array_equal(V, V0) and np.array_equal(gl, gl0) and not scal.any()
    runs = []
    for sv in (plain, StereoBASolver(prob, point_priors=None), StereoBASolver(prob, None, empty)):
        assert sv.Q is None and sv._trial.numel() == 5 and sv.point_prior_error(points) == 0.0
        sv.linearize(poses, points)
        sv.point_prior_linearize(points)
        e = sv._lm_error((poses, points))
        po, pt, rep = sv.optimize(poses, points)
        runs.append((sv.V.cpu().numpy().copy(), sv.gl.cpu().numpy().copy(), e, po.cpu().numpy(), pt.cpu().numpy(),
                     rep.err_hist, rep.lambda_hist, (rep.iterations, rep.outer, rep.tries, rep.status)))
    assert runs[0][7][0] >= 3
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_lm_walks_the_reference_lm(gpu, oracle, name):
    c = _lm_case(oracle, name)
    seq, sv = c["seq"], c["sv"]
    rposes, rpoints, rrep = c["lm"]
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    assert rrep["outer"] >= 3
    print(f"point prior LM {name}: outer {rep.outer} tries {rep.tries} error {rep.initial_error:.6g} -> {rep.final_error:.6g}; "
          f"lambda {rep.lambda_hist} vs {rrep['lambda_hist']}")
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    assert rep.initial_error == pytest.approx(rrep["initial_error"], rel=1e-11)
    e_pose, e_pt = relerr(poses.cpu().numpy(), rposes), relerr(points.cpu().numpy(), rpoints)
    print(f"point prior LM {name}: poses vs reference {e_pose:.2g}, points {e_pt:.2g}")
    assert e_pose <= 1e-6 and e_pt <= 1e-6
    assert rep.final_error < rep.initial_error
    # the priors took part: their term is in the initial error, and FAR_LM went metres towards its distant mean
    assert rep.initial_error > c["R"].prior_error(seq["points_init"]) > 10.0
    assert np.abs(points.cpu().numpy()[FAR_LM] - seq["points_gt"][FAR_LM]).max() > 1.0


def _prior_model(gtsam, sig):
    sig = np.asarray(sig, float)
    return gtsam.noiseModel.Isotropic.Sigma(3, float(sig[0])) if np.all(sig == sig[0]) else gtsam.noiseModel.Diagonal.Sigmas(sig)


def _shim_graph(seq, noise3, noise2, sensor, as_block, priors, pose_priors=(0,)):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    for i in pose_priors:
        graph.add(gtsam.PriorFactorPose3(X(i), gtsam.Pose3.from_flat12(seq["poses_gt"][i]),
                                         gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])))
    K3, K2 = gtsam.Cal3_S2Stereo(*seq["K"]), gtsam.Cal3_S2(*seq["mono_K"])
    Sp = None if sensor is None else gtsam.Pose3.from_flat12(sensor)
    for i in range(len(seq["poses_gt"])):
        values.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
    for j in range(len(seq["points_gt"])):
        values.insert(L(j), seq["points_init"][j])
    mono, meas = seq["mono"], seq["meas"]
    pk, lk = X(0) + seq["obs_pose"].astype(np.int64), L(0) + seq["obs_point"].astype(np.int64)
    for j, mean, sig in list(zip(*priors))[:3]:              # some priors before the observations, the rest after them
        graph.add(gtsam.PriorFactorPoint3(L(int(j)), mean, _prior_model(gtsam, sig)))
    if as_block:
        if (~mono).any():
            graph.push_back(gtsam.StereoFactorBlock(meas[~mono], noise3, pk[~mono], lk[~mono], K3, Sp))
        graph.push_back(gtsam.ProjectionFactorBlock(meas[mono][:, [0, 2]], noise2, pk[mono], lk[mono], K2, Sp))
    else:
        for a in range(len(meas)):
            if mono[a]:
                graph.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(meas[a, 0], meas[a, 2]), noise2,
                                                                     int(pk[a]), int(lk[a]), K2, Sp))
            else:
                graph.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*meas[a]), noise3, int(pk[a]), int(lk[a]), K3, Sp))
    for j, mean, sig in list(zip(*priors))[3:]:
        graph.add(gtsam.PriorFactorPoint3(L(int(j)), mean, _prior_model(gtsam, sig)))
    return graph, values


def _noise_models(seq, name):
    import visual_underwater_slam_amd.gtsam as gtsam
    noise3 = gtsam.noiseModel.Isotropic.Sigma(3, seq["sigma"])
    noise2 = gtsam.noiseModel.Isotropic.Sigma(2, seq["mono_sigma"])
    if LOSSES[name][0]:
        est = gtsam.noiseModel.mEstimator.Cauchy.Create(LOSSES[name][1])
        noise3, noise2 = (gtsam.noiseModel.Robust.Create(est, m) for m in (noise3, noise2))
    return noise3, noise2


def _values_arrays(values, n_kf, n_lm):
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    return (np.stack([values.atPose3(X(i)).flat12() for i in range(n_kf)]),
            np.stack([values.atPoint3(L(j)) for j in range(n_lm)]))


@pytest.mark.parametrize("name,as_block", (("gaussian", False), ("cauchy", True)))
def test_gtsam_drop_in_path(gpu, oracle, name, as_block):
    """PriorFactorPoint3 with Isotropic and Diagonal models next to single factors (Gaussian, no extrinsic) and next to
    StereoFactorBlock / ProjectionFactorBlock (Cauchy, with an extrinsic)"""
    import visual_underwater_slam_amd.gtsam as gtsam
    c = _lm_case(oracle, name)
    seq, R, priors = c["seq"], c["R"], c["priors"]
    n_kf, n_lm = len(seq["poses_gt"]), len(seq["points_gt"])
    models = [_prior_model(gtsam, s) for s in priors[2]]
    assert any(m.is_isotropic() for m in models) and not all(m.is_isotropic() for m in models)
    graph, initial = _shim_graph(seq, *_noise_models(seq, name), c["sensor"], as_block, priors)
    assert graph.nrFactors() == len(seq["meas"]) + 1 + len(priors[0])
    assert graph.error(initial) == pytest.approx(R.error(seq["poses_init"], seq["points_init"]), rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rposes, rpoints, rrep = c["lm"]
    rep = opt.report()
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    got, got_pts = _values_arrays(result, n_kf, n_lm)
    assert relerr(got, rposes) <= 1e-6 and relerr(got_pts, rpoints) <= 1e-6
    assert graph.error(result) == pytest.approx(R.error(got, got_pts), rel=1e-11)
    assert opt.error() == pytest.approx(rrep["final_error"], rel=1e-6)
    # the input Values are untouched
    p_in, x_in = _values_arrays(initial, n_kf, n_lm)
    assert np.array_equal(p_in, seq["poses_init"]) and np.array_equal(x_in, seq["points_init"])


def test_landmark_priors_fix_the_scale_of_a_monocular_graph(gpu, oracle):
    """mono factors only, PriorFactorPose3 on X(0) and PriorFactorPoint3 on two landmarks (GTSAM's SFM recipe): the
    reference's LM trajectory.  (The same graph without the landmark priors has no scale; nothing is asserted on it.)"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.ba import StereoBAProblem
    seq = mono_problem.mixed_sequence(mono_frac=1.0, n_kf=16, n_lm=80)
    assert seq["mono"].all()
    gt = seq["points_gt"]
    priors = (np.array([10, 70]), gt[[10, 70]], np.array([[0.05, 0.05, 0.05], [0.1, 0.05, 0.2]]))
    graph, initial = _shim_graph(seq, None, gtsam.noiseModel.Isotropic.Sigma(2, seq["mono_sigma"]), None, True, priors)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], 16, 80, seq["K"], seq["sigma"], mono=seq["mono"],
                           mono_K=seq["mono_K"], mono_sigma=seq["mono_sigma"])
    R = _ref(oracle, prob, seq, 0, 0.0, None, priors)
    e0 = R.error(seq["poses_init"], seq["points_init"])
    assert graph.error(initial) == pytest.approx(e0, rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rep = opt.report()
    rposes, rpoints, rrep = R.lm(seq["poses_init"], seq["points_init"])
    print(f"mono scale: outer {rep.outer} tries {rep.tries} error {rep.initial_error:.6g} -> {rep.final_error:.6g}; "
          f"reference {rrep['err_hist']}")
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    got, got_pts = _values_arrays(result, 16, 80)
    assert relerr(got, rposes) <= 1e-6 and relerr(got_pts, rpoints) <= 1e-6
    assert rep.final_error < 0.1 * e0


def test_a_prior_makes_a_single_mono_sighting_determinate_for_the_marginals(gpu, oracle):
    """at the reference LM's result: without a prior on it the landmark with one mono sighting is refused (today's
    behaviour), with one its covariance is the block of the dense f64 inverse of the reference's information matrix, at
    the 1e-9 of test_marginals_gpu.py for landmark covariances (1e-8 for the shim's joint, as there)"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    from visual_underwater_slam_amd.ba import IndeterminantSystem
    c = _lm_case(oracle, "gaussian")
    seq, sv, R, priors, lm = c["seq"], c["sv"], c["R"], c["priors"], c["single_lm"]
    rposes, rpoints, _ = c["lm"]
    poses, points = d(rposes), d(rpoints)
    keep = priors[0] != lm
    fewer = tuple(a[keep] for a in priors)
    _, sv_fewer = _problem(seq, None, None, fewer)
    with pytest.raises(IndeterminantSystem) as ei:
        sv_fewer.marginals(poses, points)
    assert (ei.value.kind, ei.value.index) == ("point", lm)
    m = sv.marginals(poses, points)
    nP = len(seq["poses_gt"])
    Hinv = np.linalg.inv(R.full_hessian(rposes, rpoints))
    blk = lambda j: Hinv[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3]
    errs = {j: relerr(m.point_cov[j].cpu().numpy(), blk(j)) for j in (lm, TRIPLE_LM, FAR_LM, 0, 79, MONO_LM)}
    e_pose = relerr(m.pose_cov[3].cpu().numpy(), Hinv[18:24, 18:24])
    print(f"point prior marginals: landmarks {errs}, pose 3 {e_pose:.2g}")
    assert max(errs.values()) < 1e-9 and e_pose < 1e-9
    # the shim: gtsam.Marginals raises gtsam's exception at the landmark, and serves it once the prior is in the graph
    noise = _noise_models(seq, "gaussian")
    result = gtsam.Values()
    for i in range(nP):
        result.insert(X(i), gtsam.Pose3.from_flat12(rposes[i]))
    for j in range(len(rpoints)):
        result.insert(L(j), rpoints[j])
    graph_fewer, _ = _shim_graph(seq, *noise, None, True, fewer)
    with pytest.raises(gtsam.IndeterminantLinearSystemException) as eg:
        gtsam.Marginals(graph_fewer, result)
    assert eg.value.key == L(lm)
    graph, _ = _shim_graph(seq, *noise, None, True, priors)
    mg = gtsam.Marginals(graph, result)
    assert relerr(mg.marginalCovariance(L(lm)), blk(lm)) < 1e-9
    assert relerr(mg.marginalCovariance(X(3)), Hinv[18:24, 18:24]) < 1e-9
    kf = int(seq["obs_pose"][seq["obs_point"] == lm][0])
    jm = mg.jointMarginalCovariance([X(kf), L(lm)])
    assert jm.keys() == [L(lm), X(kf)]                        # ascending key order: the landmark comes first
    idx = list(range(6 * nP + 3 * lm, 6 * nP + 3 * lm + 3)) + list(range(6 * kf, 6 * kf + 6))
    assert relerr(jm.fullMatrix(), Hinv[np.ix_(idx, idx)]) < 1e-8


def test_inertial_graph_with_a_landmark_prior(gpu, oracle):
    """the stereo + IMU + DVL graph of test_mono_ba_gpu.py::test_inertial_graph_takes_the_mixed_route plus one landmark
    prior, on NavBASolver: the prior's error at the result is the reference expression, and the total moved"""
    from test_nav_oracle import build_nav
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavFactors, PointPriors
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
    common = dict(prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None], pose_stride=2)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], meas, n_kf, nL, K, seq["sigma"], **common, **mk)
    lm = int(seq["obs_point"][0])
    mean, sig = seq["points_gt"][lm] + np.array([0.3, -0.2, 0.4]), np.array([0.05, 0.7, 0.2])
    with_prior = NavBASolver(prob, nav, point_priors=PointPriors([lm], mean[None], sig[None], nL))
    without = NavBASolver(prob, nav)
    assert with_prior.Q is not None and without.Q is None
    start = (d(seq["poses_init"]), d(np.zeros_like(seq["vels_gt"])), d(np.zeros(6)), d(seq["points_init"]))
    out, out0 = with_prior.optimize(*start), without.optimize(*start)
    rep, rep0 = out[4], out0[4]
    assert rep.status == 0 and np.isfinite(rep.final_error) and rep.final_error < rep.initial_error
    want0 = 0.5 * float(np.sum(((seq["points_init"][lm] - mean) / sig) ** 2))
    assert rep.initial_error - rep0.initial_error == pytest.approx(want0, rel=1e-6)
    pts = out[3].cpu().numpy()
    want = 0.5 * float(np.sum(((pts[lm] - mean) / sig) ** 2))
    got = with_prior.point_prior_error(out[3])
    print(f"inertial graph: prior error {got!r} vs {want!r}; total {rep.final_error!r} vs {rep0.final_error!r} without")
    assert got == pytest.approx(want, rel=1e-6) and want > 0.0
    total = with_prior._lm_error(out[:4])
    assert total == pytest.approx(rep.final_error, rel=1e-6)
    assert total - got == pytest.approx(with_prior.error(out[0], out[3]) + with_prior.nav_error(*out[:3]), rel=1e-12)
    assert abs(rep.final_error - rep0.final_error) > 1e-6 * rep0.final_error       # beyond the project's tolerance
    assert relerr(pts[lm], out0[3].cpu().numpy()[lm]) > 1e-4          # the prior pulled its landmark


def test_refusals(gpu):
    """vus_point_prior_check: a negative status and a vus_last_error() text for each malformed factor set; the
    landmark-sharded solver names the single-GPU solver"""
    from visual_underwater_slam_amd import _lib, dist as vdist
    from visual_underwater_slam_amd.ba import PointPriors
    lib, st = _lib.load(), _lib.current_stream_ptr()
    nL = 40
    idx = [7, 2, 7, 0, 39]
    Q = PointPriors(idx, np.arange(15.0).reshape(5, 3), 0.5 + np.arange(15.0).reshape(5, 3), nL)
    assert lib.vus_point_prior_check(Q.addr(), st) == 0
    good = {k: getattr(Q, k).clone() for k in ("row_point", "row_ptr", "mean", "w")}

    def spoil(name, index, value, word):
        getattr(Q, name)[index] = value
        rc = lib.vus_point_prior_check(Q.addr(), st)
        text = lib.vus_last_error().decode()
        getattr(Q, name).copy_(good[name])
        assert rc < 0 and word in text, (name, rc, text)
        return text

    Q.row_point[:2] = torch.tensor([2, 0], dtype=torch.int32, device="cuda")       # rows 0, 2, 7, 39 -> 2, 0, 7, 39
    rc, text = lib.vus_point_prior_check(Q.addr(), st), lib.vus_last_error().decode()
    Q.row_point.copy_(good["row_point"])
    assert rc < 0 and "ascending" in text
    spoil("row_point", 3, nL, "outside")
    spoil("row_ptr", 1, 0, "empty")
    spoil("w", (1, 2), 0.0, "weight")
    spoil("w", (4, 0), float("inf"), "weight")
    spoil("mean", (2, 0), float("nan"), "mean")
    with pytest.raises(_lib.VusError, match="mean"):
        Q.mean[0, 1] = float("nan")
        try:
            _lib.call("vus_point_prior_check", Q.addr(), st)
        finally:
            Q.mean.copy_(good["mean"])
    assert lib.vus_point_prior_check(Q.addr(), st) == 0
    # sizes and pointers are checked by every call
    bad = PointPriors(idx, np.zeros((5, 3)), np.ones((5, 3)), nL)
    bad.c.n_rows = 0
    assert lib.vus_point_prior_error(bad.addr(), None, None, None, st) < 0 and "sizes" in lib.vus_last_error().decode()
    seq = mono_problem.mixed_sequence(mono_frac=0.0, n_kf=6, n_lm=20)
    with pytest.raises(NotImplementedError, match="StereoBASolver"):
        vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, 20, seq["K"], seq["sigma"],
                                    point_priors=PointPriors([3], np.zeros((1, 3)), np.ones((1, 3)), 20))
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, 20, seq["K"], seq["sigma"])
    with pytest.raises(ValueError, match="landmarks"):
        StereoBASolver(prob, point_priors=Q)
