"""CombinedImuFactor on the GPU (NavBiasBASolver(combined=...), csrc/combined_imu.hip) against the dense f64 reference of
combined_imu_ref.py: the kernels stage by stage at 2, 6, 16 and 65 keyframes (every band mode), a mixed graph, the LM trial by
trial, the degeneration to ImuFactor + BetweenFactorConstantBias, marginals against the dense inverse, the host-side checks
and the gtsam shim end to end."""
import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
import nav_bias_ref as nbr
import combined_imu_ref as cir

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
SOLVE_C = 0.2          # solve error <= max(1e-10, SOLVE_C * kappa_s * eps), as test_nav_bias_gpu.py
COV_C = 1.0            # covariance error <= max(1e-10, COV_C * kappa_s * eps)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
WALK = (2e-3, 2e-4)    # bias random-walk step per keyframe (acc, gyro) of the test sequences, as test_nav_bias_gpu.py


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def seq(n, lm_per_kf=20, obs=40):
    return synth.nav_sequence(n, max(lm_per_kf * n, 40), obs, bias_walk_sigma=WALK)


def narrow(s):
    """The sequence with every landmark's observations cut down to its first keyframe and the next one: the landmark band is
    then one keyframe (3 nodes) and the problem's band the minimum a CombinedImuFactor asks for."""
    first = np.full(len(s["points_gt"]), 1 << 30, np.int64)
    np.minimum.at(first, s["obs_point"], s["obs_pose"])
    keep = s["obs_pose"] - first[s["obs_point"]] <= 1
    return {**s, "obs_pose": s["obs_pose"][keep], "obs_point": s["obs_point"][keep], "meas": s["meas"][keep]}


def state(s, seed=1):
    rng = np.random.default_rng(seed)
    n = len(s["poses_gt"])
    return s["poses_init"], s["vels_gt"] + 0.05 * rng.normal(size=(n, 3)), 0.01 * rng.normal(size=(n, 6)), s["points_init"]


def stage_by_stage(oracle, s, P, G, prob, sv, lam, band_tuning, modes):
    """One LM trial's kernels against the dense reference; returns the worst measured errors."""
    n, nN, B = len(s["poses_gt"]), prob.n_nodes, prob.band
    poses, vels, biases, points = state(s)
    dposes, dvels, dbiases, dpoints = d(poses), d(vels), d(biases), d(points)
    ref = cir.dense_system(oracle, s, P, G, poses, vels, biases, points, lam)      # with the combined factors (cir._factors)
    Hc, gc, ec = cir.combined_system(oracle, G, poses, vels, biases)
    worst = {}
    assert np.isclose(sv.cimu_error(dposes, dvels, dbiases), ec, rtol=1e-11)
    sv.Scimu.fill_(float("nan")); sv.gcimu.fill_(float("nan"))
    sv.cimu_linearize(dposes, dvels, dbiases)
    torch.cuda.synchronize()
    Sc = sv.Scimu.cpu().numpy()
    assert np.isfinite(Sc).all() and np.isfinite(sv.gcimu.cpu().numpy()).all()      # every block written or zeroed
    assert np.isclose(float(sv.cimu_scal[0]), ec, rtol=1e-11)
    worst["Scimu"] = relerr(Sc, nbr.band_blocks(Hc, nN, None, diagonals=6))
    worst["gcimu"] = relerr(sv.gcimu.cpu().numpy().reshape(-1), gc)
    assert worst["Scimu"] < 1e-11 and worst["gcimu"] < 1e-11, worst
    sv.nav_linearize(dposes, dvels, dbiases)
    x_ref, kappa, dsc = nbr.solve(ref["A"], -ref["g"])
    bound = max(1e-10, SOLVE_C * kappa * EPS)
    sv.linearize(dposes, dpoints)
    for mode in modes:
        band_tuning(band_mode=mode)
        sv.Sband.fill_(float("nan")); sv.gs.fill_(float("nan"))
        sv.schur(lam); sv.nav_assemble(lam); sv.cimu_assemble()
        torch.cuda.synchronize()
        Sg = sv.Sband.cpu().numpy()
        assert np.isfinite(Sg).all()
        worst["Sband"] = relerr(Sg, nbr.band_blocks(ref["A"], nN, B))
        worst["gs"] = relerr(sv.gs.cpu().numpy().reshape(-1), ref["g"])
        assert worst["Sband"] < 1e-11 and worst["gs"] < 1e-11, worst
        sv.nav_solve(lam)
        torch.cuda.synchronize()
        assert int(sv.status.item()) == 0, mode
        e = nbr.scaled_err(sv.dp.cpu().numpy().reshape(-1), x_ref, dsc)
        worst[f"solve[mode {mode}]"] = e
        assert e < bound, (mode, e, bound, kappa)
    worst["kappa_s"], worst["bound"], worst["split"] = kappa, bound, sv.use_split
    # the step's evaluation: the linearised / new errors of the combined factors (velocities and biases are retracted by
    # the inertial stage, the one writer)
    sv.dp.copy_(d(x_ref.reshape(nN, 6)))
    sv.eval_step(dposes, dpoints)
    sv.nav_eval_step(dposes, dvels, dbiases)
    sv.cimu_eval_step(dposes, dvels, dbiases)
    torch.cuda.synchronize()
    npo = sv.new_poses.cpu().numpy()
    _, dv_, _, db_ = nbr.split_step(x_ref, n)
    assert np.array_equal(sv.new_vels.cpu().numpy(), vels + dv_) and np.array_equal(sv.new_bias.cpu().numpy(), biases + db_)
    only = cir.only_combined(G)
    lin = 0.0
    for rw, cols in cir.inertial_system(oracle, only, poses, vels, biases)[3]:
        r = rw.copy()
        for node, J in cols:
            r += J @ x_ref[6 * node:6 * node + J.shape[1]]
        lin += 0.5 * float(r @ r)
    scal = sv.cimu_scal.cpu().numpy()
    assert np.isclose(scal[1], lin, rtol=1e-10), (scal[1], lin)
    assert np.isclose(scal[2], cir.inertial_error(oracle, only, npo, vels + dv_, biases + db_), rtol=1e-10)
    return worst


@pytest.mark.parametrize("n", [2, 6, 16, 65])
def test_stage_by_stage_against_the_dense_reference(oracle, band_tuning, n):
    """2 keyframes: n_nodes - 1 = 5 is the whole band; 6: the band is the minimum of 5 (the landmarks of narrow() span one
    keyframe); 16: generic; 65: a two-sided, split solve."""
    s = seq(n) if n != 6 else narrow(seq(6))
    P, G, _ = cir.make_graph(oracle, s)
    prob, sv = cir.solver(s, G)
    assert prob.n_nodes == 3 * n and prob.band >= min(5, 3 * n - 1)
    if n in (2, 6):
        assert prob.band == 5
    if n == 65:
        assert sv.use_split
    w = stage_by_stage(oracle, s, P, G, prob, sv, 1e-3, band_tuning, (0, 1, 2, 3))
    print(f"\n{n} keyframes, band {prob.band}: {w}")


def test_mixed_graph_stage_by_stage(oracle, band_tuning):
    """Combined factors on the even intervals, ImuFactor + BetweenFactorConstantBias on the odd ones."""
    s = seq(16)
    P, G, _ = cir.make_graph(oracle, s, "even")
    assert len(G.ci_i) == 8 and len(G.imu_i) == 7 and len(G.bb_i) == 7
    prob, sv = cir.solver(s, G)
    w = stage_by_stage(oracle, s, P, G, prob, sv, 1e-3, band_tuning, (0, 1, 2, 3))
    print(f"\nmixed, band {prob.band}: {w}")


@pytest.mark.parametrize("n", [16, 40])
def test_lm_takes_the_reference_trials(oracle, n):
    s = seq(n)
    P, G, _ = cir.make_graph(oracle, s)
    prob, sv = cir.solver(s, G)
    x0 = (s["poses_init"], np.zeros((n, 3)), np.zeros((n, 6)), s["points_init"])
    gp, gv, gb, gpt, grep = sv.optimize(*(d(a) for a in x0))
    rp, rv, rb, rpt, rrep = cir.lm_optimize(oracle, s, P, G, *x0)
    assert (grep.outer, grep.tries, grep.iterations, grep.status) == (rrep["outer"], rrep["tries"], rrep["iterations"],
                                                                      rrep["status"])
    assert grep.lambda_hist == rrep["lambda_hist"]
    assert abs(grep.final_error - rrep["final_error"]) < 1e-9 * rrep["final_error"]
    assert relerr(gb.cpu().numpy(), rb) < 1e-6 and relerr(gp.cpu().numpy(), rp) < 1e-8


def test_block_diagonal_covariance_is_imu_factor_plus_between(oracle):
    """Every Sigma replaced by its block diagonal (the 9 x 9 block and a diagonal 6 x 6): the combined family must then give
    the error and the step of the ImuFactor + BetweenFactorConstantBias graph with those blocks' sigmas, which nav.hip serves.
    The two systems are equal up to the order of their sums (1e-16 of a block), and a solve turns that into kappa_s eps of the
    step: at lambda = 1e-3, where kappa_s = 8.9e8, the two steps were measured 1.9e-9 apart.  The step is therefore compared at
    lambda = 1e3, where kappa_s = 2.3e5 and the solve bound of this suite, SOLVE_C kappa_s eps, is 1e-11 -- below the 1e-10
    asked of the two families (asserted from the dense reference); the step is no smaller there (max entry 0.13 against 0.16)."""
    s = seq(16)
    P, G, twin = cir.make_graph(oracle, s, degenerate=True)
    prob, sv = cir.solver(s, G)
    prob2, sv2 = nbr.solver(s, twin)
    vals = state(s)
    dv = tuple(d(v) for v in vals)
    lam = 1e3
    ref = cir.dense_system(oracle, s, P, twin, *vals, lam)
    x_ref, kappa, dsc = nbr.solve(ref["A"], -ref["g"])
    assert SOLVE_C * kappa * EPS < 1e-10 and np.abs(x_ref).max() > 0.05
    errs, steps = [], []
    for solver_, total in ((sv, lambda: sv.nav_error(*dv[:3]) + sv.cimu_error(*dv[:3])), (sv2, lambda: sv2.nav_error(*dv[:3]))):
        errs.append(total())
        solver_._lm_linearize(dv)
        solver_._lm_solve(lam)
        torch.cuda.synchronize()
        assert int(solver_.status.item()) == 0
        steps.append(solver_.dp.cpu().numpy().copy())
    assert abs(errs[0] - errs[1]) < 1e-10 * errs[1], errs
    assert relerr(steps[0], steps[1]) < 1e-10, relerr(steps[0], steps[1])
    assert relerr(steps[0].reshape(-1), x_ref) < 1e-10 and abs(errs[0] - ref["nav_err"]) < 1e-10 * ref["nav_err"]


def test_marginals_against_the_dense_inverse(oracle):
    from visual_underwater_slam_amd.ba import IndeterminantSystem
    n = 16
    s = seq(n)
    P, G, _ = cir.make_graph(oracle, s)
    assert len(G.bb_i) == 0                 # every bias but B(0) is held by combined factors alone
    prob, sv = cir.solver(s, G)
    values = state(s)
    m = sv.marginals(*(d(v) for v in values), points_cov=False)
    A = cir.dense_system(oracle, s, P, G, *values, 0.0)["A"]
    dsc = np.sqrt(np.diag(A))
    kappa = np.linalg.cond(A / dsc[:, None] / dsc[None, :])
    C = np.linalg.inv(A)
    bound = max(1e-10, COV_C * kappa * EPS)
    blk = lambda a, ra=6: C[6 * a:6 * a + ra, 6 * a:6 * a + ra]
    for name, got, want in (("pose", m.pose_cov, np.stack([blk(3 * i) for i in range(n)])),
                            ("vel", m.vel_cov, np.stack([blk(3 * i + 1, 3) for i in range(n)])),
                            ("bias", m.biases_cov, np.stack([blk(3 * i + 2) for i in range(n)]))):
        e = relerr(got.cpu().numpy(), want)
        assert e < bound, (name, e, bound, kappa)
    # without the combined factors the same NavBiasFactors leave B(1) unconstrained
    from visual_underwater_slam_amd.ba import NavBiasBASolver
    with pytest.raises(IndeterminantSystem) as e:
        NavBiasBASolver(prob, G.device()).marginals(*(d(v) for v in values), points_cov=False)
    assert (e.value.kind, e.value.index) == ("bias", 1)


def test_entry_points_check_on_the_host():
    """j != i + 1, an index out of range, band 4 and n = 0 are refused before anything is launched."""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import CombinedImuFactors
    lib = _lib.load()
    n = 4
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    B = _lib.ptr(buf)
    make = lambda: CombinedImuFactors([0, 0, -9.81], [0, 1, 2], np.zeros((3, 148)), np.tile(np.eye(15).reshape(-1), (3, 1)))
    F = make()
    assert lib.vus_cimu_error(F.addr(), n, B, B, B, B, B, None) == 0
    torch.cuda.synchronize()
    buf.zero_()

    def refused(mutate, match, n_poses=n):
        F = make()
        mutate(F)
        for call in (lambda: lib.vus_cimu_error(F.addr(), n_poses, B, B, B, B, B, None),
                     lambda: lib.vus_cimu_linearize(F.addr(), n_poses, B, B, B, B, B, B, B, None),
                     lambda: lib.vus_cimu_eval_step(F.addr(), n_poses, B, B, B, B, B, B, B, B, B, None)):
            assert call() == -1
            assert match in lib.vus_last_error().decode(), lib.vus_last_error()
    refused(lambda F: F.j.copy_(torch.tensor([1, 3, 3], dtype=torch.int32)), "CombinedImuFactor 1 joins keyframes 1 and 3")
    refused(lambda F: None, "CombinedImuFactor 2 joins keyframes 2 and 3", n_poses=3)
    refused(lambda F: F.i.copy_(torch.tensor([-1, 1, 2], dtype=torch.int32)), "CombinedImuFactor 0 joins keyframes -1")
    refused(lambda F: setattr(F.c, "n", 0), "n=0")
    assert lib.vus_cimu_assemble(3 * n, 4, B, B, B, B, None) == -1 and "band=4" in lib.vus_last_error().decode()
    torch.cuda.synchronize()
    assert not buf.any()                    # nothing was launched by a refused call
    assert lib.vus_cimu_assemble(3 * n, 5, B, B, B, B, None) == 0
    torch.cuda.synchronize()


def test_shim_end_to_end(oracle):
    """A 12-keyframe graph built with CombinedImuFactor optimises to the reference LM's values; Marginals serves it."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B
    from visual_underwater_slam_amd.gtsam.optimizer import graph_error
    n = 12
    s = seq(n)
    graph, values = cir.shim_graph(s)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, values, gtsam.LevenbergMarquardtParams())
    res = opt.optimize()
    P, G, _ = cir.make_graph(oracle, s)
    rp, rv, rb, rpt, rrep = cir.lm_optimize(oracle, s, P, G, s["poses_init"], np.zeros((n, 3)), np.zeros((n, 6)), s["points_init"])
    got_p = np.stack([res.atPose3(X(i)).flat12() for i in range(n)])
    got_v = np.stack([res.atVector(V(i)) for i in range(n)])
    got_b = np.stack([res.atConstantBias(B(i)).vector() for i in range(n)])
    assert opt.iterations() == rrep["iterations"] and abs(opt.error() - rrep["final_error"]) <= 1e-9 * rrep["final_error"]
    assert relerr(got_p, rp) < 1e-8 and relerr(got_v, rv) < 1e-6 and relerr(got_b, rb) < 1e-6
    assert np.isclose(graph_error(graph, res), rrep["final_error"], rtol=1e-9)
    mg = gtsam.Marginals(graph, res)
    jm = mg.jointMarginalCovariance([X(2), B(2), B(3)])
    assert jm.fullMatrix().shape == (18, 18) and np.allclose(jm.at(B(3), B(3)), mg.marginalCovariance(B(3)), rtol=1e-9)
    assert np.linalg.eigvalsh(mg.marginalCovariance(B(5))).min() > 0.0
