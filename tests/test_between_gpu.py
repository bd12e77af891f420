"""BetweenFactorPose3 on the MI355X (include/vus_between.h, ba.BetweenFactors, the solver hooks, the gtsam shim) against the
dense f64 reference of between_ref.py, the oracle's stereo twins and the inertial dense references."""
import numpy as np
import pytest
import torch

import between_ref as br
import marginals_ref as mr
from conftest import same_lm_trajectory
from visual_underwater_slam_amd import synth, ba_pack, _lib

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _odometry(rng, truth, pairs, noise=0.0, sig=(0.01, 0.01, 0.01, 0.05, 0.05, 0.05), losses=None):
    from visual_underwater_slam_amd.gtsam import Pose3
    meas = []
    for a, b in pairs:
        m = Pose3.from_flat12(truth[a]).between(Pose3.from_flat12(truth[b]))
        if noise:
            m = m.retract(noise * rng.standard_normal(6))
        meas.append(m.flat12())
    return br.BetweenSet([p[0] for p in pairs], [p[1] for p in pairs], np.array(meas), np.tile(sig, (len(pairs), 1)), losses)


# -- 1. the three entry points, stride 1 / 2 / 3 ----------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_stages_against_the_reference(gpu, oracle, stride):
    rng = np.random.default_rng(10 + stride)
    n = 30
    truth, init, _, _ = br.pose_graph(rng, n)
    # both key orders, a duplicate pair, a long one; robust on some factors: with the Gaussian odometry, all six kinds
    pairs = [(k - 1, k) for k in range(1, n)] + [(5, 2), (2, 5), (2, 5), (29, 3), (10, 24), (17, 13)]
    losses = [(0, 0.0)] * (n - 1) + [(2, 0.5), (0, 0.0), (1, 0.3), (5, 1.0), (3, 2.0), (4, 1.5)]
    G = _odometry(rng, truth, pairs, noise=0.02, losses=losses)
    B = G.device(n, pose_stride=stride)
    nN, band = stride * n, stride * G.span
    poses = d(init)
    lin = torch.empty((B.n, 120), dtype=torch.float64, device="cuda")
    sc = torch.zeros(4, dtype=torch.float64, device="cuda")
    work = torch.empty(int(_lib.load().vus_between_work_doubles(B.addr())), dtype=torch.float64, device="cuda")
    st = _lib.current_stream_ptr()
    p = _lib.ptr
    _lib.call("vus_between_check", B.addr(), band, st)
    _lib.call("vus_between_linearize", B.addr(), p(poses), p(lin), p(sc), p(work), st)
    H, g, e0, fac = br.system(oracle, G, init, nN, stride)
    assert relerr(sc[0].item(), e0) < 1e-12
    runs = []
    for _ in range(2):
        Sb = torch.zeros((nN, band + 1, 36), dtype=torch.float64, device="cuda")
        gs = torch.zeros((nN, 6), dtype=torch.float64, device="cuda")
        _lib.call("vus_between_assemble", B.addr(), p(lin), band, p(Sb), p(gs), st)
        runs.append((Sb.cpu().numpy(), gs.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])     # bit-identical
    Sref = mr.dense_to_band(H, band).reshape(nN, band + 1, 36)
    assert relerr(runs[0][0], Sref) < 1e-12
    assert relerr(runs[0][1].reshape(-1), g) < 1e-12
    # eval at a step: linearised error at the old poses, error at the retracted ones
    x = 0.01 * rng.standard_normal(6 * nN)
    new = np.stack([oracle.pose_retract(init[k], x[6 * stride * k:6 * stride * k + 6]) for k in range(n)])
    dp, new_d = d(x.reshape(nN, 6)), d(new)          # held: a temporary's memory would be reused by the next one
    _lib.call("vus_between_eval_step", B.addr(), p(poses), p(dp), p(new_d), p(sc[1:]), p(work), st)
    out = sc.cpu().numpy()
    assert relerr(out[1], br.linear_error(fac, x, stride)) < 1e-12
    assert relerr(out[2], br.error(oracle, G, new)) < 1e-12
    err = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib.call("vus_between_error", B.addr(), p(poses), p(err), p(work), st)
    assert relerr(err.item(), br.error(oracle, G, init)) < 1e-12


def _stereo(n_kf, n_lm, obs, seed=3):
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    n, nL = n_kf, len(seq["points_gt"])
    return seq, n, nL


def _oracle_problem(oracle, seq, n, nL):
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]),
                                   torch.from_numpy(seq["meas"]), n, nL)
    return oracle.BAProblem(pk, seq["K"], seq["sigma"], (np.array([0], np.int32), seq["poses_init"][:1], seq["prior_sigmas"][None]))


def _gpu_stereo(seq, n, nL, G, loss=None):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                           prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=G.span)
    return prob, StereoBASolver(prob, G.device(n))


def test_schur_plus_between_writes_every_block_of_a_widened_band(gpu, oracle):
    """A between span wider than the landmark span: the band follows it, and after schur + assemble every stored block of
    the NaN-prefilled Sband has been written and equals the dense reference."""
    import nav_ref
    seq, n, nL = _stereo(200, 3000, 300)
    lm_span = nav_ref.pose_band(seq["obs_pose"], seq["obs_point"])
    assert lm_span + 20 < n
    rng = np.random.default_rng(1)
    pairs = [(k - 1, k) for k in range(1, n)] + [(0, lm_span + 20), (45, 5)]
    G = _odometry(rng, seq["poses_gt"], pairs, noise=0.01)
    prob, sv = _gpu_stereo(seq, n, nL, G)
    assert prob.band == G.span > lm_span
    P = _oracle_problem(oracle, seq, n, nL)
    lam = 1e-3
    sv.linearize(d(seq["poses_init"]), d(seq["points_init"]))
    sv.between_linearize(d(seq["poses_init"]))
    sv.Sband.fill_(float("nan"))
    sv.schur(lam)
    sv.between_assemble()
    Sb = sv.Sband.cpu().numpy()
    for i in range(n):
        assert np.isfinite(Sb[i, :min(i, prob.band) + 1]).all(), i
    A, g, _, _ = br.stereo_dense(oracle, P, seq["poses_init"], seq["points_init"], prob.band, lam)
    H, gb, _, _ = br.system(oracle, G, seq["poses_init"], n)
    want = mr.dense_to_band(A + H, prob.band).reshape(n, prob.band + 1, 36)
    for i in range(n):
        s = min(i, prob.band) + 1
        assert relerr(Sb[i, :s], want[i, :s]) < 1e-10, i
    assert relerr(sv.gs.cpu().numpy().reshape(-1), g + gb) < 1e-10


# -- 2. / 3. pose-only LM ----------------------------------------------------------------------------------------------
def _pose_only(n, closures, noise, loss=None, seed=7):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    rng = np.random.default_rng(seed)
    truth, init, G, priors = br.pose_graph(rng, n, closures=closures, noise=noise, loss=loss)
    z = np.zeros((0,))
    prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                           prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=G.span)
    return truth, init, G, priors, prob, StereoBASolver(prob, G.device(n))


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_pose_graph_lm_walks_the_dense_lm(gpu, oracle, noise):
    truth, init, G, priors, prob, sv = _pose_only(60, [(0, 59), (10, 40), (30, 5)], noise)
    poses, _, rep = sv.optimize(d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    ref, _, orep = br.lm_optimize(oracle, G, init, priors=priors)
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    got = poses.cpu().numpy()
    assert relerr(got, ref) < 1e-6
    assert abs(rep.final_error - orep["final_error"]) <= 1e-6 * max(orep["final_error"], 1e-9) + 1e-12
    if noise == 0.0:
        assert np.abs(got - truth).max() < 1e-6


def test_long_closure_runs_in_per_panel_launch_mode(gpu, oracle):
    lib = _lib.load()
    truth, init, G, priors, prob, sv = _pose_only(400, [(0, 399), (50, 300)], 0.0)
    assert prob.band == 399
    poses, _, rep = sv.optimize(d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    assert lib.vus_ba_get_tuning(_lib.TUNE_LAST_BAND_MODE) != 3     # per-panel launches, not the persistent window kernel
    ref, _, orep = br.lm_optimize(oracle, G, init, priors=priors)
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    assert relerr(poses.cpu().numpy(), ref) < 1e-6
    assert np.abs(poses.cpu().numpy() - truth).max() < 1e-6


# -- 4. stereo + between, and the inertial solvers ---------------------------------------------------------------------
def test_stereo_plus_between_lm(gpu, oracle):
    seq, n, nL = _stereo(200, 3000, 300)
    rng = np.random.default_rng(2)
    pairs = [(k - 1, k) for k in range(1, n)] + [(3, 9), (120, 112)]
    G = _odometry(rng, seq["poses_gt"], pairs, noise=0.005)
    prob, sv = _gpu_stereo(seq, n, nL, G)
    P = _oracle_problem(oracle, seq, n, nL)
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    ref, rpts, orep = br.lm_optimize(oracle, G, seq["poses_init"], P=P, points=seq["points_init"], band=prob.band)
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    assert relerr(poses.cpu().numpy(), ref) < 1e-6
    assert relerr(points.cpu().numpy(), rpts) < 1e-6


@pytest.mark.parametrize("stride", [2, 3])
def test_inertial_solvers_with_between_factors(gpu, oracle, stride):
    """The first trial's camera-side system and step of NavBASolver / NavBiasBASolver with between factors equal the
    inertial dense references plus the between blocks; the LM then converges with a monotone error."""
    import nav_ref
    import nav_bias_ref as nbr
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver
    s = synth.nav_sequence(16, 300, 60)
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    rng = np.random.default_rng(3)
    G = _odometry(rng, s["poses_gt"], [(k - 1, k) for k in range(1, n)] + [(0, 12), (14, 2)], noise=0.01)
    vels, lam = np.zeros((n, 3)), 1e-3
    if stride == 3:
        P, NG = nbr.make_graph(oracle, s)
        prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                               prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=3,
                               between_span=G.span)
        from visual_underwater_slam_amd.ba import NavBiasBASolver
        sv = NavBiasBASolver(prob, NG.device(), G.device(n, 3))
        bias = np.zeros((n, 6))
        ref = nbr.dense_system(oracle, s, P, NG, s["poses_init"], vels, bias, s["points_init"], lam, band=prob.band // 3)
        A, g = ref["A"], ref["g"]
    else:
        from test_nav_oracle import build_nav
        from visual_underwater_slam_amd.ba import NavFactors
        P, _ = build_nav(oracle, s)
        pims, Ws = nbr.preintegrate(s)
        imu = (np.arange(n - 1), np.arange(1, n), pims, Ws)
        dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
        vpr = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
        N = oracle.NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr)
        prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                               prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=2,
                               between_span=G.span)
        sv = NavBASolver(prob, NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr), G.device(n, 2))
        bias = np.zeros(6)
        ref = nav_ref.dense_system(oracle, s, P, N, s["poses_init"], vels, bias, s["points_init"], lam)
        A, g = ref["A"], ref["g"]
    nc = 6 * stride * n
    H, gb, _, _ = br.system(oracle, G, s["poses_init"], stride * n, stride)
    A = A.copy(); g = g.copy()
    A[:nc, :nc] += H
    g[:nc] += gb
    state = (d(s["poses_init"]), d(vels), d(bias), d(s["points_init"]))
    sv._lm_linearize(state)
    sv._lm_solve(lam)
    x = np.linalg.solve(A, -g)
    assert relerr(sv.dp.cpu().numpy().reshape(-1), x[:nc]) < 1e-7
    *_, rep = sv.optimize(*state)
    assert rep.status == 0 and all(b <= a * (1 + 1e-12) for a, b in zip(rep.err_hist, rep.err_hist[1:]))
    assert rep.final_error < rep.initial_error


# -- 5. a robust closure ------------------------------------------------------------------------------------------------
def test_robust_closure_survives_a_false_loop_closure(gpu, oracle):
    from visual_underwater_slam_amd.gtsam import Pose3
    rng = np.random.default_rng(9)
    n = 40
    truth, init, G, priors = br.pose_graph(rng, n, closures=[(0, 39), (5, 30)], noise=0.002)
    wrong = Pose3.from_flat12(truth[10]).between(Pose3.from_flat12(truth[35])).retract(np.array([0.5, -0.4, 0.3, 3.0, -2.0, 1.5]))
    results = {}
    for name, loss in (("gauss", (0, 0.0)), ("cauchy", (2, 1.0)), ("huber", (1, 1.345))):
        Gk = br.BetweenSet(np.r_[G.i, 10], np.r_[G.j, 35], np.vstack([G.meas, wrong.flat12()]), np.vstack([1.0 / G.w, 1.0 / G.w[:1]]),
                           [(0, 0.0)] * (n - 1) + [loss] * 3)
        from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
        z = np.zeros((0,))
        prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]),
                               1.0, prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=Gk.span)
        sv = StereoBASolver(prob, Gk.device(n))
        poses, _, rep = sv.optimize(d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
        ref, _, orep = br.lm_optimize(oracle, Gk, init, priors=priors)
        same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
        assert relerr(poses.cpu().numpy(), ref) < 1e-6, name
        results[name] = np.abs(poses.cpu().numpy()[:, 9:] - truth[:, 9:]).max()
    # measured (seed 9): Gaussian 3.43 m off the truth, Huber 0.41 m, Cauchy 0.083 m (odometry noise alone drifts cm)
    assert results["cauchy"] < 0.05 * results["gauss"] and results["huber"] < 0.2 * results["gauss"], results
    assert results["gauss"] > 1.0, results


# -- 6. / 7. the gtsam shim ---------------------------------------------------------------------------------------------
def _shim_graph(seq, n, G, stereo=True):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(seq["poses_init"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])))
    for f in range(len(G.i)):
        graph.add(gtsam.BetweenFactorPose3(X(int(G.i[f])), X(int(G.j[f])), gtsam.Pose3.from_flat12(G.meas[f]),
                                           gtsam.noiseModel.Diagonal.Sigmas(1.0 / G.w[f])))
    for k in range(n):
        values.insert(X(k), gtsam.Pose3.from_flat12(seq["poses_init"][k]))
    if stereo:
        K = gtsam.Cal3_S2Stereo(*seq["K"])
        noise = gtsam.noiseModel.Isotropic.Sigma(3, seq["sigma"])
        for j in range(len(seq["points_gt"])):
            values.insert(L(j), seq["points_init"][j])
        for a in range(len(seq["obs_pose"])):
            graph.add(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*seq["meas"][a]), noise, X(int(seq["obs_pose"][a])),
                                                  L(int(seq["obs_point"][a])), K))
    return graph, values


def test_gtsam_drop_in(gpu, oracle):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    seq, n, nL = _stereo(12, 300, 60)
    rng = np.random.default_rng(4)
    G = _odometry(rng, seq["poses_gt"], [(k - 1, k) for k in range(1, n)] + [(11, 0)], noise=0.005)
    graph, values = _shim_graph(seq, n, G)
    P = _oracle_problem(oracle, seq, n, nL)
    e = graph.error(values)
    want = oracle.ba_error(P, seq["poses_init"], seq["points_init"]) + br.error(oracle, G, seq["poses_init"])
    assert relerr(e, want) < 1e-10 and br.error(oracle, G, seq["poses_init"]) > 1e-3 * e
    opt = gtsam.LevenbergMarquardtOptimizer(graph, values, gtsam.LevenbergMarquardtParams())
    res = opt.optimize()
    ref, _, orep = br.lm_optimize(oracle, G, seq["poses_init"], P=P, points=seq["points_init"], band=n - 1)
    got = np.stack([res.atPose3(X(k)).flat12() for k in range(n)])
    assert relerr(got, ref) < 1e-6
    rep = opt.report()
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)


def test_marginals_with_between_factors(gpu, oracle):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    rng = np.random.default_rng(6)
    truth, init, G, priors = br.pose_graph(rng, 30, closures=[(0, 29), (4, 20)], noise=0.01)
    seq = {"poses_init": init, "prior_sigmas": 1.0 / priors[2][0]}
    graph, values = _shim_graph(seq, 30, G, stereo=False)
    m = gtsam.Marginals(graph, values)
    Hb, _, _, _ = br.system(oracle, G, init, 30)
    Hp, _, _ = br.prior_system(oracle, priors, init)
    Ainv = np.linalg.inv(Hb + Hp)
    for k in (0, 7, 29):
        assert relerr(m.marginalCovariance(X(k)), Ainv[6 * k:6 * k + 6, 6 * k:6 * k + 6]) < 1e-8
    J = m.jointMarginalCovariance([X(4), X(20)]).fullMatrix()
    idx = list(range(24, 30)) + list(range(120, 126))
    assert relerr(J, Ainv[np.ix_(idx, idx)]) < 1e-8


# -- 8. scale ------------------------------------------------------------------------------------------------------------
def test_configs2_with_odometry(gpu):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    n_kf, n_lm, obs = synth.CONFIGS2_BA
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    n, nL = n_kf, len(seq["points_gt"])
    rng = np.random.default_rng(8)
    G = _odometry(rng, seq["poses_gt"], [(k - 1, k) for k in range(1, n)], noise=0.002)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                           prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=G.span)
    sv = StereoBASolver(prob, G.device(n))
    _, _, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    assert rep.status == 0
    assert all(b <= a for a, b in zip(rep.err_hist, rep.err_hist[1:]))
    assert rep.final_error < rep.initial_error
