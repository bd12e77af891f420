"""Position and attitude fixes on keyframe poses on the MI355X (include/vus_pose_meas.h, ba.PoseMeasurements, the solver
hooks, the gtsam shim) against the numpy reference tests/pose_meas_ref.py and the 60-digit fixture
tests/golden/pose_meas_general_position.npz: the raw entry points, the workgroup boundary and determinism, the stages in
the solver, the LM, the no-op guarantee, the gauge, inertial graphs, the drop-in path and the refusals."""
import os

import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
from conftest import same_lm_trajectory
import general_position
import mono_problem
import pose_meas_ref as pmr
import sensor_ref

pytestmark = pytest.mark.gpu

S = sensor_ref.extrinsic()
LOSSES = {"gaussian": (0, 0.0), "cauchy": (2, 2.3849)}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_meas_general_position.npz")
OUTPUTS = ("Hpp", "gp", "err", "eval", "error", "weights")
NO_PRIORS = (np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 3)))


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw_calls(M, poses, dp, new_poses, Hpp, gp):
    """the five entry points called directly on copies of Hpp / gp: (Hpp, gp, [err, lin, new, error], weights) as numpy"""
    from visual_underwater_slam_amd import _lib
    p, st = _lib.ptr, _lib.current_stream_ptr()
    Hpp, gp = Hpp.clone(), gp.clone()
    scal = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    w = torch.full((max(M.n, 1),), 7.0, dtype=torch.float64, device="cuda")
    work = torch.empty((int(_lib.load().vus_pose_meas_work_doubles(M.addr())),), dtype=torch.float64, device="cuda")
    _lib.call("vus_pose_meas_linearize", M.addr(), p(poses), p(Hpp), p(gp), p(scal), p(work), st)
    _lib.call("vus_pose_meas_eval_step", M.addr(), p(poses), p(dp), p(new_poses), p(scal[1:]), p(work), st)
    _lib.call("vus_pose_meas_error", M.addr(), p(poses), p(scal[3:]), p(work), st)
    _lib.call("vus_pose_meas_weights", M.addr(), p(poses), p(w), st)
    return Hpp.cpu().numpy(), gp.cpu().numpy(), scal.cpu().numpy(), w.cpu().numpy()[:M.n]


# -- 1 ------------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_on_the_general_position_fixture(gpu):
    """every block of the Hpp / gp increments, the four scalars and the weights within tol_block of the 60-digit reference"""
    from visual_underwater_slam_amd import _lib
    c = dict(np.load(FIXTURE))
    G = pmr.PoseMeasSet(c["idx"], c["kind"], c["meas"], c["sigmas"], list(zip(c["loss_kind"].tolist(), c["loss_k"].reshape(-1).tolist())))
    nP = len(c["poses"])
    M = G.device(nP)
    _lib.call("vus_pose_meas_check", M.addr(), _lib.current_stream_ptr())
    Hpp, gp, scal, w = _raw_calls(M, d(c["poses"]), d(c["dp"]), d(c["new_poses"]), torch.zeros((nP, 36), dtype=torch.float64, device="cuda"),
                                  torch.zeros((nP, 6), dtype=torch.float64, device="cuda"))
    got = {"Hpp": Hpp, "gp": gp, "err": scal[0:1, None], "eval": scal[1:3, None], "error": scal[3:4, None], "weights": w[:, None]}
    r = general_position.ratios(got, c, OUTPUTS)
    print("pose_meas fixture, |gpu - want| / tol_block:", {k: f"{v:.3g}" for k, v in r.items()})
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(r.values()) <= 1.0, r
    assert not Hpp[6].any() and not gp[6].any()               # the pose without a factor


# -- 2 ------------------------------------------------------------------------------------------------------------------
def _many_rows(nP):
    """nP poses in general position, a factor on every one given in DESCENDING pose order, five factors of both kinds on
    pose 3 in the middle of the list, the six losses in turn"""
    U = synth._hash_uniform
    a3 = np.arange(3 * nP, dtype=np.int64)
    poses = np.zeros((nP, 12))
    w = 2.0 * (U(a3, 21).reshape(nP, 3) - 0.5)
    t = 40.0 * (U(a3, 22).reshape(nP, 3) - 0.5)
    for i in range(nP):
        poses[i] = np.concatenate([pmr.so3_exp(w[i]).reshape(9), t[i]])
    idx = list(range(nP - 1, -1, -1))
    idx[150:150] = [3, 3, 3, 3]
    n = len(idx)
    an = np.arange(3 * n, dtype=np.int64)
    kind = (np.arange(n) % 3 == 1).astype(np.int64)
    assert set(kind[np.array(idx) == 3].tolist()) == {0, 1} and idx.count(3) == 5
    sig = np.where(kind[:, None] == 1, 0.02 + 0.2 * U(an, 23).reshape(n, 3), 0.05 + 3.0 * U(an, 24).reshape(n, 3))
    arm, noise, wr = U(an, 25).reshape(n, 3) - 0.5, 3.0 * sig * (U(an, 26).reshape(n, 3) - 0.5), 2.5 * (U(an, 27).reshape(n, 3) - 0.5)
    meas = np.array([pmr.rotation_meas(poses[idx[f]], wr[f]) if kind[f] else
                     pmr.position_meas(poses[idx[f]], arm[f] if f % 2 else np.zeros(3), noise[f]) for f in range(n)])
    losses = [(f % 6, 0.0 if f % 6 == 0 else 0.5 + 2.0 * float(U(np.array([f]), 28)[0])) for f in range(n)]
    return poses, pmr.PoseMeasSet(idx, kind, meas, sig, losses)


@pytest.mark.parametrize("rows", (256, 257, 310))
@pytest.mark.parametrize("stride", (1, 2, 3))
def test_many_rows_cross_the_workgroup_boundary_and_two_runs_are_bit_identical(gpu, stride, rows):
    """256, 257 or 310 factor-carrying poses (exactly one workgroup of 256 rows; a second one with a single live row; more
    than one and no multiple of it) on arbitrary Hpp / gp, with the step on the pose nodes of a stride-1, 2 or 3 layout
    (the other nodes hold NaN): the increments, the four scalars and the weights against the reference, and every output of
    two calls on the same inputs bit for bit"""
    from visual_underwater_slam_amd import _lib
    poses, G = _many_rows(rows)
    nP = len(poses)
    M = G.device(nP, pose_stride=stride)
    assert (M.n, M.n_rows) == (nP + 4, nP) and nP == rows and (np.diff(G.idx) < 0).any()
    _lib.call("vus_pose_meas_check", M.addr(), _lib.current_stream_ptr())
    assert int(_lib.load().vus_pose_meas_work_doubles(M.addr())) >= 4
    U = synth._hash_uniform
    a6 = np.arange(6 * nP, dtype=np.int64)
    dpp = (U(a6, 31).reshape(nP, 6) - 0.5) * np.array([0.1, 0.1, 0.1, 1.0, 1.0, 1.0])
    dp = np.full((stride * nP, 6), np.nan)
    dp[::stride] = dpp
    new_poses = np.stack([np.concatenate([(poses[i, :9].reshape(3, 3) @ pmr.so3_exp(0.5 * dpp[i, :3])).reshape(9),
                                          poses[i, 9:] + 0.5 * dpp[i, 3:]]) for i in range(nP)])
    Hpp0 = 50.0 * (U(np.arange(36 * nP, dtype=np.int64), 32).reshape(nP, 36) - 0.5)
    gp0 = 10.0 * (U(a6, 33).reshape(nP, 6) - 0.5)
    args = (M, d(poses), d(dp), d(new_poses), d(Hpp0), d(gp0))
    Hpp, gp, scal, w = _raw_calls(*args)
    H, g, e0, fac = pmr.blocks(G, poses)
    want = [e0, pmr.linear_error(fac, dpp), pmr.error(G, new_poses), pmr.error(G, poses)]
    errs = {"Hpp": relerr(Hpp - Hpp0, H), "gp": relerr(gp - gp0, g), "w": relerr(w, pmr.weights(G, poses)[G.csr_order()])}
    print(f"pose measurements, {M.n_rows} rows, stride {stride}: {errs}; scalars {scal.tolist()} vs {want}")
    assert np.isfinite(Hpp).all() and np.isfinite(gp).all() and np.isfinite(scal).all()
    assert max(errs.values()) <= 1e-11
    assert np.allclose(scal, want, rtol=1e-11, atol=0)
    assert relerr((Hpp - Hpp0)[3], H[3]) <= 1e-11 and np.abs(H[3]).max() > 0           # the five factors of pose 3
    Hpp2, gp2, scal2, w2 = _raw_calls(*args)
    assert np.array_equal(Hpp, Hpp2) and np.array_equal(gp, gp2) and np.array_equal(scal, scal2) and np.array_equal(w, w2)


# -- the solver scenes ----------------------------------------------------------------------------------------------------
def _problem(seq, loss, sensor, G=None, pose_priors=(0,), **kw):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    nP = len(seq["poses_gt"])
    pp = list(pose_priors)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], nP, len(seq["points_gt"]), seq["K"], seq["sigma"],
                           prior_pose=pp, prior_T=seq["poses_gt"][pp], prior_sigmas=np.tile(seq["prior_sigmas"], (len(pp), 1)),
                           loss=loss if loss and loss[0] else None, body_P_sensor=sensor, mono=seq["mono"], mono_K=seq["mono_K"],
                           mono_sigma=seq["mono_sigma"])
    return prob, StereoBASolver(prob, pose_meas=None if G is None else G.device(nP), **kw)


def _ref(oracle, prob, seq, kind, k, sensor, G, pose_priors=(0,)):
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    perm = pk["perm"].numpy().astype(np.int64)
    pp = np.array(pose_priors, np.int64)
    return pmr.PoseMeasBA(oracle, pk, seq["K"], seq["sigma"], kind, k, sensor, np.asarray(seq["mono"])[perm], seq["mono_K"],
                          seq["mono_sigma"], (pp, seq["poses_gt"][pp], np.tile(seq["prior_sigmas"], (len(pp), 1))),
                          point_priors=None, pose_meas=G)


# -- 3 ------------------------------------------------------------------------------------------------------------------
def test_stages_in_the_solver(gpu, oracle):
    """mixed_sequence() (70 keyframes / 310 landmarks) with an extrinsic, mono rows and Cauchy; position fixes (some with
    lever arms, Cauchy, one displaced) on every third body pose, depth-only fixes on every fifth, rotation fixes on every
    seventh: Hpp, gp and the term's slot after _lm_linearize, the three totals after one trial, at 1e-11"""
    kind, k = LOSSES["cauchy"]
    seq = sensor_ref.body_sequence(mono_problem.mixed_sequence(outliers=0.05), S)
    G, pos = pmr.fix_set(seq["poses_gt"], loss=(2, 2.0), displaced=(2,))
    assert len(pos) == 24 and (G.meas[G.kind == 0, 3:6] != 0).any() and (G.kind == 1).sum() == 10
    assert (G.sigmas[:, 2] == 0.02).sum() == 14 and (np.diff(G.idx) < 0).any()
    prob, sv = _problem(seq, (kind, k), S, G)
    assert sv._loss_args("vus_ba_linearize")[0] == "vus_ba_linearize_mixed" and sv.M.n == G.n and sv._trial.numel() == 9
    R = _ref(oracle, prob, seq, kind, k, S, G)
    p0, x0 = seq["poses_init"], seq["points_init"]
    state = (d(p0), d(x0))
    sv.linearize(*state)
    H0, g0, obs0 = sv.Hpp.cpu().numpy().copy(), sv.gp.cpu().numpy().copy(), float(sv.scal[0])
    sv._lm_linearize(state)
    lin = R.linearize(p0, x0)
    Hpp, gp = sv.Hpp.cpu().numpy(), sv.gp.cpu().numpy()
    Hm, gm, em, _ = pmr.blocks(G, p0)
    errs = {"Hpp": relerr(Hpp, lin["Hpp"]), "gp": relerr(gp, lin["gp"]), "dHpp": relerr(Hpp - H0, Hm), "dgp": relerr(gp - g0, gm)}
    print(f"pose measurement stages: {errs}; slot {float(sv.pm_scal[0])!r} vs {lin['pm_err']!r}")
    assert max(errs.values()) <= 1e-11
    assert float(sv.scal[0]) == obs0 and float(sv.pm_scal[0]) == pytest.approx(lin["pm_err"], rel=1e-11)
    rest = np.setdiff1d(np.arange(len(p0)), G.idx)
    assert len(rest) and np.array_equal(Hpp[rest], H0[rest]) and np.array_equal(gp[rest], g0[rest])
    sv.schur(1e-3); sv.band_solve(); sv.backsub()
    status, sc = sv._lm_eval(state)
    dp, dl = sv.dp.cpu().numpy(), sv.dl.cpu().numpy()
    npo, npt = R.retract(p0, x0, dp, dl)
    want = [lin["err"], R.linear_error(dp, dl), R.error(npo, npt)]
    got = [float(x) for x in sv.pm_scal.cpu()]
    print(f"pose measurement stages: totals {sc} vs {want}; term {got[:3]}")
    assert status == 0 and np.allclose(sc, want, rtol=1e-11, atol=0)
    assert got[1] == pytest.approx(R.pose_meas_linear_error(dp), rel=1e-11) and got[2] == pytest.approx(pmr.error(G, npo), rel=1e-11)
    assert want[1] < want[0]
    assert sv.pose_meas_error(state[0]) == pytest.approx(pmr.error(G, p0), rel=1e-11)
    assert sv._lm_error(state) == pytest.approx(R.error(p0, x0), rel=1e-11)
    wts = sv.pose_meas_weights(state[0]).cpu().numpy()          # graph order
    assert relerr(wts, pmr.weights(G, p0)) <= 1e-11 and wts[pos[2]] < 0.1 and (wts[G.kind == 1] == 1.0).all()


# -- 4 ------------------------------------------------------------------------------------------------------------------
LM_CASES = {"gaussian": (None, 0.0, ()), "cauchy": (S, 0.10, (4, 11))}        # extrinsic, stereo outliers, displaced fixes
_lm_cache = {}


def _lm_sequence(sensor, outliers):
    seq = mono_problem.mixed_sequence(n_kf=16, n_lm=80, outliers=outliers)
    return seq if sensor is None else sensor_ref.body_sequence(seq, sensor)


def _lm_case(oracle, name):
    """problem, solver, reference and the reference LM of one case, computed once and shared (read only): a position fix
    on every keyframe (2 of 16 displaced by 5 - 30 m in the Cauchy case), depth fixes on every fifth, rotation fixes on
    every seventh"""
    if name not in _lm_cache:
        sensor, outliers, displaced = LM_CASES[name]
        seq = _lm_sequence(sensor, outliers)
        loss = LOSSES[name]
        G, pos = pmr.fix_set(seq["poses_gt"], every_pos=1, loss=loss if loss[0] else None, displaced=displaced)
        prob, sv = _problem(seq, loss, sensor, G)
        R = _ref(oracle, prob, seq, *loss, sensor, G)
        _lm_cache[name] = dict(seq=seq, G=G, pos=pos, displaced=[pos[q] for q in displaced], prob=prob, sv=sv, R=R, sensor=sensor,
                               lm=R.lm(seq["poses_init"], seq["points_init"]))
    return _lm_cache[name]


@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_lm_walks_the_reference_lm(gpu, oracle, name):
    """Gaussian; and Cauchy with 2 of the 16 position fixes displaced by 5 - 30 m: the reference's trajectory, and the final
    weights of the displaced fixes < 0.1, of the others > 0.5 (the reference alone satisfies this split: asserted first)"""
    c = _lm_case(oracle, name)
    seq, sv, G = c["seq"], c["sv"], c["G"]
    rposes, rpoints, rrep = c["lm"]
    assert len(c["pos"]) == 16 and rrep["outer"] >= 3 and rrep["status"] == 0
    rw = pmr.weights(G, rposes)
    out = np.zeros(G.n, bool)
    out[c["displaced"]] = True
    if name == "cauchy":
        assert out.sum() == 2 and rw[out].max() < 0.1 and rw[~out].min() > 0.5, (rw[out], rw[~out].min())
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    print(f"pose measurement LM {name}: outer {rep.outer} tries {rep.tries} error {rep.initial_error:.6g} -> {rep.final_error:.6g}; "
          f"lambda {rep.lambda_hist} vs {rrep['lambda_hist']}")
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    assert rep.initial_error == pytest.approx(rrep["initial_error"], rel=1e-11)
    e_pose, e_pt = relerr(poses.cpu().numpy(), rposes), relerr(points.cpu().numpy(), rpoints)
    print(f"pose measurement LM {name}: poses vs reference {e_pose:.2g}, points {e_pt:.2g}")
    assert e_pose <= 1e-6 and e_pt <= 1e-6 and rep.final_error < rep.initial_error
    assert rep.initial_error > pmr.error(G, seq["poses_init"]) > 1.0               # the fixes took part
    w = sv.pose_meas_weights(poses).cpu().numpy()
    if name == "cauchy":
        print(f"final weights: displaced {w[out]}, the rest >= {w[~out].min():.3f}")
        assert w[out].max() < 0.1 and w[~out].min() > 0.5
    else:
        assert (w == 1.0).all()


# -- 5 ------------------------------------------------------------------------------------------------------------------
def test_no_factors_is_a_no_op(gpu):
    """n == 0 at the C ABI (sums 0, Hpp / gp untouched) and pose_meas=None / an empty PoseMeasurements in the solver: stages
    and a whole optimize() bit-identical to the solver built without the argument, the trial record of length 5 (the
    16-keyframe case, whose LM is reproducible bit for bit: test_point_prior_gpu.py::test_no_priors_is_a_no_op)"""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import PoseMeasurements, StereoBASolver
    seq = _lm_sequence(None, 0.0)
    nP = len(seq["poses_gt"])
    empty = PoseMeasurements([], [], np.zeros((0, 9)), np.zeros((0, 3)), nP)
    _lib.call("vus_pose_meas_check", empty.addr(), _lib.current_stream_ptr())
    prob, _ = _problem(seq, None, None)
    plain = StereoBASolver(prob)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    plain.linearize(poses, points)
    H0, g0 = plain.Hpp.cpu().numpy().copy(), plain.gp.cpu().numpy().copy()
    Hpp, gp, scal, w = _raw_calls(empty, poses, plain.dp.zero_(), poses, plain.Hpp, plain.gp)
    assert np.array_equal(Hpp, H0) and np.array_equal(gp, g0) and not scal.any() and len(w) == 0
    runs = []
    for sv in (plain, StereoBASolver(prob, pose_meas=None), StereoBASolver(prob, None, None, (), empty)):
        assert sv.M is None and sv._trial.numel() == 5 and sv.pose_meas_error(poses) == 0.0 and sv.pose_meas_weights(poses) is None
        sv.linearize(poses, points)
        sv.pose_meas_linearize(poses)
        sv.pose_meas_eval_step(poses)
        e = sv._lm_error((poses, points))
        po, pt, rep = sv.optimize(poses, points)
        runs.append((sv.Hpp.cpu().numpy().copy(), sv.gp.cpu().numpy().copy(), e, po.cpu().numpy(), pt.cpu().numpy(),
                     rep.err_hist, rep.lambda_hist, (rep.iterations, rep.outer, rep.tries, rep.status)))
    assert runs[0][7][0] >= 3
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(np.asarray(x), np.asarray(y))


# -- 6 ------------------------------------------------------------------------------------------------------------------
def test_position_fixes_alone_fix_the_gauge(gpu, oracle):
    """a stereo graph without any PriorFactorPose3: marginals() raises IndeterminantSystem; with position fixes on four
    keyframes whose positions are not collinear it succeeds, the pose covariances are blocks of the dense inverse of the
    reference's full Hessian (1e-8) and optimize() converges"""
    from visual_underwater_slam_amd.ba import IndeterminantSystem
    seq = mono_problem.mixed_sequence(mono_frac=0.0, n_kf=16, n_lm=80)
    nP = len(seq["poses_gt"])
    kf = np.array([0, 3, 9, 15])
    t = seq["poses_gt"][kf, 9:]
    sv_ = np.linalg.svd(t - t.mean(0), compute_uv=False)
    print(f"singular values of the centred fix positions: {sv_}")
    assert sv_[1] > 0.02 and sv_[1] > 0.02 * sv_[0]             # not collinear: the rotation about their line is observable
    sig = np.full((4, 3), 0.02)
    noise = 0.02 * (synth._hash_uniform(np.arange(12, dtype=np.int64), 91).reshape(4, 3) - 0.5)
    G = pmr.PoseMeasSet(kf[::-1], [0] * 4, [pmr.position_meas(seq["poses_gt"][i], np.zeros(3), noise[q]) for q, i in enumerate(kf[::-1])], sig)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    _, free = _problem(seq, None, None, None, pose_priors=())
    with pytest.raises(IndeterminantSystem):
        free.marginals(poses, points)
    prob, sv = _problem(seq, None, None, G, pose_priors=())
    po, pt, rep = sv.optimize(poses, points)
    assert rep.status == 0 and rep.iterations >= 2 and rep.final_error < rep.initial_error
    R = _ref(oracle, prob, seq, 0, 0.0, None, G, pose_priors=())
    m = sv.marginals(po, pt)
    rposes, rpoints = po.cpu().numpy(), pt.cpu().numpy()
    Hinv = np.linalg.inv(R.full_hessian(rposes, rpoints))
    errs = [relerr(m.pose_cov[i].cpu().numpy(), Hinv[6 * i:6 * i + 6, 6 * i:6 * i + 6]) for i in range(nP)]
    print(f"gauge from position fixes: LM {rep.initial_error:.4g} -> {rep.final_error:.4g}, pose covariances vs dense inverse {max(errs):.2g}")
    assert max(errs) < 1e-8


# -- 7 ------------------------------------------------------------------------------------------------------------------
def _depth_fixes(seq):
    nP = len(seq["poses_gt"])
    noise = np.zeros((nP, 3))
    noise[:, 2] = 0.04 * (synth._hash_uniform(np.arange(nP, dtype=np.int64), 92) - 0.5)
    return pmr.PoseMeasSet(np.arange(nP)[::-1], [0] * nP, [pmr.position_meas(seq["poses_gt"][i], np.zeros(3), noise[i]) for i in range(nP)][::-1],
                           np.tile([1e3, 1e3, 0.02], (nP, 1)))


@pytest.mark.parametrize("stride", (2, 3))
def test_inertial_graphs_with_depth_fixes(gpu, oracle, stride):
    """NavBASolver (stride 2) and NavBiasBASolver (stride 3) on nav_sequence(10, 200, 50) with a depth fix on every
    keyframe: the term in the initial error, the error at the result and its split into terms"""
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavBiasBASolver, NavFactors
    seq = synth.nav_sequence(10, 200, 50)
    n_kf, nL = len(seq["poses_gt"]), len(seq["points_gt"])
    G = _depth_fixes(seq)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, nL, seq["K"], seq["sigma"], prior_pose=[0],
                           prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None], pose_stride=stride)
    if stride == 2:
        from test_nav_oracle import build_nav
        _, N = build_nav(oracle, seq, zero_velocity_prior=False)
        nav = NavFactors(seq["gravity"], imu=(N.imu_i, N.imu_j, N.imu_pim, N.imu_W), dvl=(N.dvl_pose, N.dvl_meas, 1.0 / N.dvl_w),
                         vprior=(N.vp_idx, N.vp_v, 1.0 / N.vp_w))
        make = lambda **kw: NavBASolver(prob, nav, **kw)
        bias0 = np.zeros(6)
    else:
        import nav_bias_ref as nbr
        _, BG = nbr.make_graph(oracle, seq)
        nav = BG.device()
        make = lambda **kw: NavBiasBASolver(prob, nav, **kw)
        bias0 = np.zeros((n_kf, 6))
    with_fix, without = make(pose_meas=G.device(n_kf, pose_stride=stride)), make()
    assert with_fix.M is not None and without.M is None and with_fix._trial.numel() == without._trial.numel() + 4
    with pytest.raises(ValueError, match="pose_stride"):
        make(pose_meas=G.device(n_kf, pose_stride=1))
    start = (d(seq["poses_init"]), d(np.zeros_like(seq["vels_gt"])), d(bias0), d(seq["points_init"]))
    out, out0 = with_fix.optimize(*start), without.optimize(*start)
    rep, rep0 = out[4], out0[4]
    assert rep.status == 0 and np.isfinite(rep.final_error) and rep.final_error < rep.initial_error
    want0 = pmr.error(G, seq["poses_init"])
    assert rep.initial_error - rep0.initial_error == pytest.approx(want0, rel=1e-6) and want0 > 0.0
    got, want = with_fix.pose_meas_error(out[0]), pmr.error(G, out[0].cpu().numpy())
    print(f"inertial graph, stride {stride}: depth-fix error {got!r} vs {want!r}; total {rep.final_error!r} vs {rep0.final_error!r} without")
    assert got == pytest.approx(want, rel=1e-6)
    total = with_fix._lm_error(out[:4])
    assert total == pytest.approx(rep.final_error, rel=1e-6)
    assert total - got == pytest.approx(with_fix.error(out[0], out[3]) + with_fix.nav_error(*out[:3]), rel=1e-12)
    # the fixes pulled the depths: closer to the measured z than without them
    z = lambda o: np.abs(o[0].cpu().numpy()[G.idx, 11] - G.meas[:, 2]).max()
    assert z(out) < z(out0)


# -- 8 ------------------------------------------------------------------------------------------------------------------
def _add_fixes(graph, G):
    """the factor set through the four shim classes, in graph order"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    made = set()
    for f in range(G.n):
        sig = G.sigmas[f]
        model = gtsam.noiseModel.Isotropic.Sigma(3, float(sig[0])) if np.all(sig == sig[0]) else gtsam.noiseModel.Diagonal.Sigmas(sig)
        if G.losses[f][0]:
            assert G.losses[f][0] == 2
            model = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Cauchy.Create(G.losses[f][1]), model)
        key, m9 = X(int(G.idx[f])), G.meas[f]
        if G.kind[f] == pmr.ROTATION:
            fac = gtsam.PoseRotationPrior3D(key, gtsam.Rot3(m9.reshape(3, 3)), model)
        elif m9[3:6].any():
            fac = gtsam.GPSFactorArm(key, m9[:3], m9[3:6], model)
        elif f % 2:
            fac = gtsam.PoseTranslationPrior3D(key, gtsam.Pose3(gtsam.Rot3(), m9[:3]), model)
        else:
            fac = gtsam.GPSFactor(key, gtsam.Point3(*m9[:3]), model)
        made.add(type(fac).__name__)
        graph.add(fac)
    return made


@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_gtsam_drop_in_path(gpu, oracle, name):
    """the scene of the LM test through GPSFactor, GPSFactorArm, PoseTranslationPrior3D, PoseRotationPrior3D and
    LevenbergMarquardtOptimizer: the solver-level result, graph.error() and report().pose_meas_weights"""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    from test_point_prior_gpu import _shim_graph, _noise_models, _values_arrays
    c = _lm_case(oracle, name)
    seq, R, G, sv = c["seq"], c["R"], c["G"], c["sv"]
    n_kf, n_lm = len(seq["poses_gt"]), len(seq["points_gt"])
    graph, initial = _shim_graph(seq, *_noise_models(seq, name), c["sensor"], name == "cauchy", NO_PRIORS)
    assert _add_fixes(graph, G) == {"GPSFactor", "GPSFactorArm", "PoseTranslationPrior3D", "PoseRotationPrior3D"}
    assert graph.nrFactors() == len(seq["meas"]) + 1 + G.n
    assert graph.error(initial) == pytest.approx(R.error(seq["poses_init"], seq["points_init"]), rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rep = opt.report()
    rposes, rpoints, rrep = c["lm"]
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    got, got_pts = _values_arrays(result, n_kf, n_lm)
    assert relerr(got, rposes) <= 1e-6 and relerr(got_pts, rpoints) <= 1e-6
    # the solver-level run of the same factors (the rows reach the packer in another order: equal to round-off, not bitwise)
    sposes, spoints, srep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    assert (rep.outer, rep.tries, rep.status) == (srep.outer, srep.tries, srep.status)
    assert np.allclose(rep.err_hist, srep.err_hist, rtol=1e-9, atol=0)
    assert relerr(got, sposes.cpu().numpy()) <= 1e-9 and relerr(got_pts, spoints.cpu().numpy()) <= 1e-9
    assert graph.error(result) == pytest.approx(R.error(got, got_pts), rel=1e-11)
    assert opt.error() == pytest.approx(rrep["final_error"], rel=1e-6)
    if name == "cauchy":
        keys, w = rep.pose_meas_weights
        assert keys.tolist() == [X(int(i)) for i in G.idx] and relerr(w, pmr.weights(G, got)) <= 1e-9
        assert w[c["displaced"]].max() < 0.1 and rep.stereo_weights is not None
    else:
        assert rep.pose_meas_weights is None
    p_in, x_in = _values_arrays(initial, n_kf, n_lm)
    assert np.array_equal(p_in, seq["poses_init"]) and np.array_equal(x_in, seq["points_init"])


# -- 9 ------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    """vus_pose_meas_check: a negative status and a vus_last_error() word for each malformed factor set; sizes and pointers
    in every call; a PoseMeasurements built for another problem; the landmark-sharded solver names the single-GPU solver"""
    from visual_underwater_slam_amd import _lib, dist as vdist
    from visual_underwater_slam_amd.ba import PoseMeasurements, StereoBAProblem, StereoBASolver
    lib, st = _lib.load(), _lib.current_stream_ptr()
    nP = 40
    idx, kind = [7, 2, 7, 0, 39], [0, 1, 1, 0, 0]
    Rm = pmr.so3_exp([0.3, -0.2, 0.5]).reshape(9)
    meas = np.array([np.r_[1.0, 2.0, 3.0, 0.1, 0.2, 0.3, 0, 0, 0], Rm, Rm, np.r_[4.0, 5.0, 6.0, np.zeros(6)], np.r_[7.0, 8.0, 9.0, np.zeros(6)]])
    M = PoseMeasurements(idx, kind, meas, 0.5 + np.arange(15.0).reshape(5, 3), nP, loss=[None, ("huber", 1.3), None, ("tukey", 4.0), None])
    assert lib.vus_pose_meas_check(M.addr(), st) == 0
    assert M.kind.tolist() == [0, 1, 0, 1, 0]                  # CSR order: poses 0, 2, 7, 7, 39
    names = ("row_pose", "row_ptr", "kind", "meas", "w", "loss_kind", "loss_k")
    good = {k: getattr(M, k).clone() for k in names}

    def spoil(name, index, value, word):
        getattr(M, name)[index] = value
        rc = lib.vus_pose_meas_check(M.addr(), st)
        text = lib.vus_last_error().decode()
        getattr(M, name).copy_(good[name])
        assert rc < 0 and word in text, (name, rc, text)

    M.row_pose[:2] = torch.tensor([2, 0], dtype=torch.int32, device="cuda")         # rows 0, 2, 7, 39 -> 2, 0, 7, 39
    rc, text = lib.vus_pose_meas_check(M.addr(), st), lib.vus_last_error().decode()
    M.row_pose.copy_(good["row_pose"])
    assert rc < 0 and "ascending" in text
    spoil("row_ptr", 1, 0, "empty")
    spoil("row_pose", 3, nP, "outside")
    spoil("kind", 2, 2, "kind")
    spoil("w", (1, 2), 0.0, "weight")
    spoil("w", (4, 0), float("inf"), "weight")
    spoil("meas", (0, 4), float("nan"), "finite")
    spoil("meas", (1, 0), float(Rm[0]) + 1e-6, "orthonormal")
    M.meas[3] = torch.from_numpy(Rm.reshape(3, 3) @ np.diag([1.0, 1.0, -1.0])).reshape(9).cuda()
    rc, text = lib.vus_pose_meas_check(M.addr(), st), lib.vus_last_error().decode()
    M.meas.copy_(good["meas"])
    assert rc < 0 and "reflection" in text
    spoil("loss_kind", 1, 6, "loss kind")
    assert M.loss_kind.tolist() == [3, 1, 0, 0, 0]
    spoil("loss_k", 0, 0.0, "loss parameter")
    spoil("loss_k", 1, float("nan"), "loss parameter")
    with pytest.raises(_lib.VusError, match="finite"):
        M.meas[0, 1] = float("nan")
        try:
            _lib.call("vus_pose_meas_check", M.addr(), st)
        finally:
            M.meas.copy_(good["meas"])
    assert lib.vus_pose_meas_check(M.addr(), st) == 0
    # sizes and pointers are checked by every call
    bad = PoseMeasurements(idx, kind, meas, np.ones((5, 3)), nP)
    bad.c.n_rows = 0
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")      # never reached: every call below is refused on the host
    p = _lib.ptr(buf)
    for call in (lambda: lib.vus_pose_meas_check(bad.addr(), st), lambda: lib.vus_pose_meas_linearize(bad.addr(), p, p, p, p, p, st),
                 lambda: lib.vus_pose_meas_eval_step(bad.addr(), p, p, p, p, p, st), lambda: lib.vus_pose_meas_error(bad.addr(), p, p, p, st),
                 lambda: lib.vus_pose_meas_weights(bad.addr(), p, p, st)):
        assert call() < 0 and "sizes" in lib.vus_last_error().decode()
    bad.c.n_rows = 4
    bad.c.pose_stride = 4
    assert lib.vus_pose_meas_error(bad.addr(), p, p, p, st) < 0 and "sizes" in lib.vus_last_error().decode()
    bad.c.pose_stride = 1
    assert lib.vus_pose_meas_linearize(bad.addr(), p, None, p, p, p, st) < 0 and "null" in lib.vus_last_error().decode()
    assert lib.vus_pose_meas_eval_step(bad.addr(), p, None, p, p, p, st) < 0 and "null" in lib.vus_last_error().decode()
    assert lib.vus_pose_meas_error(bad.addr(), p, None, p, st) < 0 and "null" in lib.vus_last_error().decode()
    assert lib.vus_pose_meas_weights(bad.addr(), None, p, st) < 0 and "null" in lib.vus_last_error().decode()
    bad.c.w = None
    assert lib.vus_pose_meas_error(bad.addr(), p, p, p, st) < 0 and "null" in lib.vus_last_error().decode()
    assert lib.vus_pose_meas_error(None, p, p, p, st) < 0
    # a set built for another problem
    seq = mono_problem.mixed_sequence(mono_frac=0.0, n_kf=6, n_lm=20)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, 20, seq["K"], seq["sigma"])
    fix = lambda **kw: PoseMeasurements([3], [0], np.zeros((1, 9)), np.ones((1, 3)), **kw)
    with pytest.raises(ValueError, match="pose_stride"):
        StereoBASolver(prob, pose_meas=fix(n_poses=6, pose_stride=2))
    with pytest.raises(ValueError, match="poses"):
        StereoBASolver(prob, pose_meas=fix(n_poses=7))
    assert StereoBASolver(prob, pose_meas=fix(n_poses=6)).M.n == 1
    with pytest.raises(NotImplementedError, match="StereoBASolver"):
        vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, 20, seq["K"], seq["sigma"],
                                    pose_meas=fix(n_poses=6))
