"""Full-covariance noise models on BetweenFactorPose3 on the MI355X (vus_between_factors.sqrt_info: between.hip, closure.hip,
ba.BetweenFactors, the gtsam shim, sequence.LoopClosureParams(noise="full")) against the dense f64 reference of
between_gauss_ref.py, which whitens with the same R.  Covariances are Q diag(s^2) Q^T of condition 1e4, seeded, and one
measured by the front end on the closed track of loop_scene.py (the two whole-solve comparisons of the long path use
correlated covariances of condition 975: _long_against_wide says why).  Tolerances are those of test_between_gpu.py for the same
stages: 1e-12 single stages, 1e-10 after the Schur step, 1e-6 LM results, 1e-8 marginals.  The diagonal path is held to
the bits it gave before the field existed (tests/golden/between_diag_bits.npz)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import between_ref as br
import between_gauss_ref as bg
import closure_ref as cr
import marginals_ref as mr
from conftest import same_lm_trajectory
from visual_underwater_slam_amd import synth, ba_pack, _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def no_points():
    return torch.zeros((0, 3), dtype=torch.float64, device="cuda")


# ---- the front end's own covariance -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_track(gpu):
    """The closed track of loop_scene.py through run_sequence with the default (diagonal) closures, once: its inputs, its
    stages and the covariance loop_closure_measurements gives for the revisit."""
    import loop_scene as S
    from visual_underwater_slam_amd import sequence
    from visual_underwater_slam_amd.frontend import ImageProcessorParams
    gt = S.poses_gt()
    frames = synth.scene_frames(gt, S.H, S.W, xp=torch, device="cuda").contiguous()
    T, n_per = 0.2, 40
    rate = S.YAW_END / (S.N_KF - 1) / T
    imu = [np.tile(np.array([0.0, 0.0, -synth.GRAVITY, 0.0, 0.0, -rate]), (n_per, 1)) for _ in range(S.N_KF - 1)]
    vel = np.diff(gt[:, 9:], axis=0) / T
    dvl = np.stack([gt[k, :9].reshape(3, 3).T @ vel[min(k, S.N_KF - 2)] for k in range(S.N_KF)])
    prm = ImageProcessorParams(max_features=S.KP, **sequence.SEQUENCE_PARAMS)
    args = (frames, S.poses_drifted(gt), imu, dvl)
    lc = sequence.LoopClosureParams()
    res, seq, st = sequence.run_sequence(*args, disparity_sign=1, params=prm, loop_closure=lc)
    acc, _, cov, _ = sequence.loop_closure_measurements(st["loop_result"], lc)
    pairs = list(zip(*(x.tolist() for x in st["loop_pairs"])))
    c = pairs.index(S.REVISIT)
    assert acc[c]
    return dict(args=args, params=prm, gt=gt, result=res, stages=st, seq=seq, cov=cov[c].copy())


def test_the_measured_covariance_is_a_full_model(loop_track):
    C = loop_track["cov"]
    s = np.sqrt(np.diag(C))
    corr = C / np.outer(s, s)
    off = np.abs(corr - np.eye(6))
    print(f"revisit covariance: sigmas {s.tolist()}, condition {np.linalg.cond(C):.3g}, largest correlation {off.max():.4f} at "
          f"{np.unravel_index(off.argmax(), off.shape)}")
    from visual_underwater_slam_amd import gtsam
    assert np.abs(C - C.T).max() <= 1e-9 * np.abs(C).max() and np.linalg.eigvalsh(C).min() > 0
    assert isinstance(gtsam.noiseModel.Gaussian.Covariance(C), gtsam.noiseModel.Gaussian) and off.max() > 0


# ---- sets ----------------------------------------------------------------------------------------------------------------
def full_set(rng, truth, pairs, noise=0.02, losses=None, real=None, cov=None):
    """A GaussSet measured from `truth` with tangent noise under seeded covariances of condition 1e4 (or cov(f) for factor
    f when `cov` is given); the last factor carries the covariance `real` when one is given."""
    from visual_underwater_slam_amd.gtsam import Pose3
    meas = [Pose3.from_flat12(truth[a]).between(Pose3.from_flat12(truth[b])).retract(noise * rng.standard_normal(6)).flat12()
            for a, b in pairs]
    covs = [bg.random_covariance(rng) if cov is None else cov(f) for f in range(len(pairs))]
    if real is not None:
        covs[-1] = real
    return bg.GaussSet([p[0] for p in pairs], [p[1] for p in pairs], np.array(meas), bg.sqrt_info(np.stack(covs)), losses)


def stage_buffers(B):
    lin = torch.empty((B.n, 120), dtype=torch.float64, device="cuda")
    sc = torch.zeros(4, dtype=torch.float64, device="cuda")
    work = torch.empty(int(_lib.load().vus_between_work_doubles(B.addr())), dtype=torch.float64, device="cuda")
    return lin, sc, work


# ---- 1. the entry points against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_stages_against_the_reference(gpu, oracle, loop_track, stride):
    rng = np.random.default_rng(110 + stride)
    n = 30
    truth, init, _, _ = br.pose_graph(rng, n)
    # both key orders, two factors on one pair, a long one; Cauchy and Huber over full models next to Gaussian ones
    pairs = [(k - 1, k) for k in range(1, n)] + [(5, 2), (2, 5), (2, 5), (29, 3), (10, 24), (17, 13)]
    losses = [(0, 0.0)] * (n - 1) + [(2, 0.5), (0, 0.0), (1, 0.3), (2, 1.0), (1, 1.345), (0, 0.0)]
    G = full_set(rng, truth, pairs, losses=losses, real=loop_track["cov"])
    B = G.device(n, pose_stride=stride)
    nN, band = stride * n, stride * G.span
    poses = d(init)
    lin, sc, work = stage_buffers(B)
    st, p = _lib.current_stream_ptr(), _lib.ptr
    _lib.call("vus_between_check", B.addr(), band, st)
    _lib.call("vus_between_linearize", B.addr(), p(poses), p(lin), p(sc), p(work), st)
    H, g, e0, fac = bg.system(oracle, G, init, nN, stride)
    e_lin, e_err = relerr(lin.cpu().numpy(), bg.lin_rows(fac)), relerr(sc[0].item(), e0)
    runs = []
    for _ in range(2):
        Sb = torch.zeros((nN, band + 1, 36), dtype=torch.float64, device="cuda")
        gs = torch.zeros((nN, 6), dtype=torch.float64, device="cuda")
        _lib.call("vus_between_assemble", B.addr(), p(lin), band, p(Sb), p(gs), st)
        runs.append((Sb.cpu().numpy(), gs.cpu().numpy()))
    Sref = mr.dense_to_band(H, band).reshape(nN, band + 1, 36)
    e_S, e_g = relerr(runs[0][0], Sref), relerr(runs[0][1].reshape(-1), g)
    x = 0.01 * rng.standard_normal(6 * nN)
    new = np.stack([oracle.pose_retract(init[k], x[6 * stride * k:6 * stride * k + 6]) for k in range(n)])
    dp, new_d = d(x.reshape(nN, 6)), d(new)
    _lib.call("vus_between_eval_step", B.addr(), p(poses), p(dp), p(new_d), p(sc[1:]), p(work), st)
    out = sc.cpu().numpy()
    err = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib.call("vus_between_error", B.addr(), p(poses), p(err), p(work), st)
    e_ev = (relerr(out[1], bg.linear_error(fac, x, stride)), relerr(out[2], bg.error(oracle, G, new)),
            relerr(err.item(), bg.error(oracle, G, init)))
    print(f"stride {stride}: lin {e_lin:.2e}, err {e_err:.2e}, Sband {e_S:.2e}, gs {e_g:.2e}, eval / new / error {e_ev}")
    assert e_lin < 1e-12 and e_err < 1e-12 and e_S < 1e-12 and e_g < 1e-12 and max(e_ev) < 1e-12
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])     # bit-identical
    # J2^T J2 is a full block now: its off-diagonal entries are there
    assert np.abs(lin.cpu().numpy()[:, 72:108].reshape(-1, 6, 6)[:, 0, 1]).min() > 0


@pytest.mark.parametrize("count", [1, 256, 257])
def test_factor_counts_around_a_workgroup(gpu, oracle, count):
    """One thread, a full workgroup of 256, one factor into the second workgroup."""
    rng = np.random.default_rng(120 + count)
    n = 20
    truth, init, _, _ = br.pose_graph(rng, n)
    a = rng.integers(0, n, count)
    b = (a + rng.integers(1, n, count)) % n                     # any other pose: both key orders, repeated pairs
    kinds = [(0, 0.0), (2, 0.5), (1, 0.3)]
    G = full_set(rng, truth, list(zip(a.tolist(), b.tolist())), losses=[kinds[f % 3] for f in range(count)])
    B = G.device(n)
    band = max(G.span, 1)
    lin, sc, work = stage_buffers(B)
    lin.fill_(float("nan"))
    poses = d(init)
    st, p = _lib.current_stream_ptr(), _lib.ptr
    _lib.call("vus_between_check", B.addr(), band, st)
    _lib.call("vus_between_linearize", B.addr(), p(poses), p(lin), p(sc), p(work), st)
    H, g, e0, fac = bg.system(oracle, G, init, n)
    assert relerr(lin.cpu().numpy(), bg.lin_rows(fac)) < 1e-12 and relerr(sc[0].item(), e0) < 1e-12
    Sb = torch.zeros((n, band + 1, 36), dtype=torch.float64, device="cuda")
    gs = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    _lib.call("vus_between_assemble", B.addr(), p(lin), band, p(Sb), p(gs), st)
    assert relerr(Sb.cpu().numpy(), mr.dense_to_band(H, band).reshape(n, band + 1, 36)) < 1e-12
    assert relerr(gs.cpu().numpy().reshape(-1), g) < 1e-12
    x = 0.01 * rng.standard_normal(6 * n)
    new = np.stack([oracle.pose_retract(init[k], x[6 * k:6 * k + 6]) for k in range(n)])
    dp, new_d = d(x.reshape(n, 6)), d(new)
    _lib.call("vus_between_eval_step", B.addr(), p(poses), p(dp), p(new_d), p(sc[1:]), p(work), st)
    out = sc.cpu().numpy()
    assert relerr(out[1], bg.linear_error(fac, x)) < 1e-12 and relerr(out[2], bg.error(oracle, G, new)) < 1e-12


def _pose_only(G, priors, n, max_span=None):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    bf = G.device(n, max_span=max_span)
    z = np.zeros((0,))
    prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                           prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=bf.span)
    return prob, StereoBASolver(prob, bf)


def _stereo(n_kf, n_lm, obs):
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    return seq, n_kf, len(seq["points_gt"])


def _oracle_problem(oracle, seq, n, nL):
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]),
                                   torch.from_numpy(seq["meas"]), n, nL)
    return oracle.BAProblem(pk, seq["K"], seq["sigma"], (np.array([0], np.int32), seq["poses_init"][:1], seq["prior_sigmas"][None]))


def test_assemble_into_a_nan_prefilled_schur_output(gpu, oracle):
    """Stereo + full between factors whose span widens the band: after schur + assemble every stored block of the
    NaN-prefilled Sband is written and equals the dense reference (1e-10, after the Schur step)."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    import nav_ref
    seq, n, nL = _stereo(40, 600, 120)
    lm_span = nav_ref.pose_band(seq["obs_pose"], seq["obs_point"])
    rng = np.random.default_rng(130)
    far = min(lm_span + 5, n - 1)
    G = full_set(rng, seq["poses_gt"], [(k - 1, k) for k in range(1, n)] + [(0, far), (25, 5)], noise=0.01)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                           prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=G.span)
    sv = StereoBASolver(prob, G.device(n))
    assert prob.band == G.span >= lm_span
    P = _oracle_problem(oracle, seq, n, nL)
    lam = 1e-3
    sv.linearize(d(seq["poses_init"]), d(seq["points_init"]))
    sv.between_linearize(d(seq["poses_init"]))
    sv.Sband.fill_(float("nan"))
    sv.schur(lam)
    sv.between_assemble()
    Sb = sv.Sband.cpu().numpy()
    A, g, _, _ = br.stereo_dense(oracle, P, seq["poses_init"], seq["points_init"], prob.band, lam)
    H, gb, _, _ = bg.system(oracle, G, seq["poses_init"], n)
    want = mr.dense_to_band(A + H, prob.band).reshape(n, prob.band + 1, 36)
    for i in range(n):
        s = min(i, prob.band) + 1
        assert np.isfinite(Sb[i, :s]).all(), i
        assert relerr(Sb[i, :s], want[i, :s]) < 1e-10, i
    assert relerr(sv.gs.cpu().numpy().reshape(-1), g + gb) < 1e-10


# ---- 2. the diagonal path ---------------------------------------------------------------------------------------------------
def _golden():
    spec = importlib.util.spec_from_file_location("make_between_diag_fixture", os.path.join(HERE, "golden", "make_between_diag_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(os.path.join(HERE, "golden", "between_diag_bits.npz"))
    c = {k: z[k] for k in z.files if not k.startswith("out_")}
    return mod, c, {k[4:]: z[k] for k in z.files if k.startswith("out_")}


def test_diagonal_sets_give_the_bits_they_gave_before(gpu):
    """The stored inputs through today's kernels without sqrt_info: lin, Sband, gs, the errors and the long path's rows equal
    the arrays captured before full-covariance models existed, bit for bit."""
    mod, c, want = _golden()
    got = mod.run(c)
    assert set(got) == set(want) == {"lin", "lin_err", "Sband", "gs", "eval", "error", "rows", "rows_err"}
    for k in want:
        assert got[k].dtype == want[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (k, relerr(got[k], want[k]))
    assert np.abs(want["lin"]).max() > 0 and np.abs(want["Sband"]).max() > 0


def test_diagonal_models_given_as_sqrt_info_agree_with_the_sigmas(gpu):
    """sqrt_info = diag(1 / sigma) against the same set given as sigmas, 1e-13 relative, every output."""
    mod, c, want = _golden()
    R = np.stack([np.diag(1.0 / s) for s in c["sigmas"]])
    got = mod.run(c, sqrt_info=R)
    err = {k: relerr(got[k], want[k]) for k in want}
    print(err)
    assert max(err.values()) < 1e-13, err
    J2 = got["rows"][:, 36:72].reshape(-1, 6, 6)
    assert not J2[:, ~np.eye(6, dtype=bool)].any() and np.array_equal(J2, want["rows"][:, 36:72].reshape(-1, 6, 6))


# ---- 3. the long path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_closure_stage_kernels_with_full_models(gpu, oracle, stride):
    from test_closure_gpu import factor, resolve
    rng = np.random.default_rng(140 + stride)
    n, M = 30, 5
    truth, init, _, _ = br.pose_graph(rng, n)
    long_pairs = [(2, 20), (20, 2), (2, 20), (2, 27), (10, 16), (25, 8)]
    long_losses = [(2, 0.5), (0, 0.0), (1, 0.3), (2, 1.0), (0, 0.0), (1, 1.345)]
    pairs = [(k - 1, k) for k in range(1, n)] + [(3, 7)] + long_pairs
    G = full_set(rng, truth, pairs, losses=[(0, 0.0)] * n + long_losses)
    bf = G.device(n, stride, max_span=M)
    far = np.abs(G.i - G.j) > M
    Glong = bg.GaussSet(G.i[far], G.j[far], G.meas[far], G.R[far], [l for l, f in zip(G.losses, far) if f])
    Lg = bf.long
    assert bf.n == n and Lg.n == 6 and np.array_equal(Lg.host["sqrt_info"], Glong.R)
    nN, band, m = stride * n, stride * M, 36
    st, p = _lib.current_stream_ptr(), _lib.ptr
    _lib.call("vus_closure_check", Lg.addr(), band, st)
    poses = d(init)
    f64 = dict(dtype=torch.float64, device="cuda")
    rows, sc = torch.full((6, 78), float("nan"), **f64), torch.zeros(4, **f64)
    work = torch.empty(int(_lib.load().vus_closure_work_doubles(Lg.addr())), **f64)
    _lib.call("vus_closure_linearize", Lg.addr(), p(poses), p(rows), p(sc), p(work), st)
    H, g, e0, fac = bg.system(oracle, Glong, init, nN, stride)
    R = rows.cpu().numpy()
    assert relerr(R, cr.rows(fac)) < 1e-12 and abs(sc[0].item() - e0) < 1e-12 * e0
    J2 = R[:, 36:72].reshape(-1, 6, 6)
    assert not np.tril(J2, -1).any() and (J2[:, np.triu_indices(6)[0], np.triu_indices(6)[1]] != 0).all()   # sw R, zeros written
    gs = torch.zeros((nN, 6), **f64)
    _lib.call("vus_closure_gradient", Lg.addr(), p(rows), p(gs), st)
    assert relerr(gs.cpu().numpy().reshape(-1), g) < 1e-12
    U = torch.full((m, 6 * nN), float("nan"), **f64)
    _lib.call("vus_closure_scatter", Lg.addr(), p(rows), p(U), st)
    want = np.zeros((m, 6 * nN))
    for f, (a, b) in enumerate(long_pairs):
        want[6 * f:6 * f + 6, 6 * stride * a:6 * stride * a + 6] = R[f, :36].reshape(6, 6)
        want[6 * f:6 * f + 6, 6 * stride * b:6 * stride * b + 6] = R[f, 36:72].reshape(6, 6)
    Un = U.cpu().numpy()
    assert np.array_equal(Un, want)
    assert relerr(Un.T @ Un, H) < 1e-12                            # U U^T is the long set's information
    # capacitance and correction on a band system of the size of U U^T (the rule of test_closure_gpu.py)
    A, Sb = mr.random_spd_band(rng, nN, band)
    scale = np.abs(Un.T @ Un).max() / np.abs(A).max()
    A, Sb = scale * A, scale * Sb
    b = rng.normal(size=(2, 6 * nN))
    X = d(b)
    d_L = factor(Sb, band, X)
    resolve(d_L, nN, band, U, m)
    C = torch.empty((m, m), **f64)
    _lib.call("vus_closure_capacitance", Lg.addr(), p(rows), p(U), p(C), st)
    _lib.call("vus_closure_correct", Lg.addr(), p(rows), p(U), p(C), p(X), 2, p(work), st)
    xref = np.linalg.solve(A + Un.T @ Un, b.T).T
    e_x = relerr(X.cpu().numpy(), xref)
    print(f"stride {stride}: corrected columns {e_x:.2e}, cond {np.linalg.cond(A + Un.T @ Un):.2e}")
    assert e_x <= 1e-11


LAM = 1e-3


def _trial(sv, state):
    sv._lm_linearize(state)
    sv._lm_solve(LAM)
    assert int(sv.status.item()) == 0
    return sv.dp.cpu().numpy().reshape(-1)


def _long_against_wide(oracle, n, closures, seed):
    """One trial at LAM of a pose graph under full models, its closures long (a low-rank term) and in a widened band:
    (dp long, dp wide, dense solve, number of long closures).

    The covariances here correlate one rotation with one translation component by +-0.95 (condition 975), not the seeded
    condition-1e4 family of the stage tests: a comparison of two f64 solves at 1e-9 needs a system whose condition times
    2^-53 stays under that.  Worked out on the CPU with numpy alone (40 poses, 2 closures): the seeded family gives
    cond(S) = 5.6e10, where numpy's dense solve and numpy's own low-rank solve (closure_ref.lowrank_solve) are 2.7e-4
    apart; this family gives cond(S) = 3.8e7 and 5.4e-9 between the same two numpy solves."""
    rng = np.random.default_rng(seed)
    truth, init, _, priors = br.pose_graph(rng, n)
    G = full_set(rng, truth, [(k - 1, k) for k in range(1, n)] + list(closures), noise=0.01,
                 cov=lambda f: bg.correlated_covariance(0.95 if f % 2 else -0.95))
    A0, g0, _ = br.prior_system(oracle, priors, init)
    H, g, _, _ = bg.system(oracle, G, init, n)
    ref = np.linalg.solve(A0 + LAM * np.eye(6 * n) + H, -(g0 + g))
    state = (d(init), no_points())
    prob_l, sv_l = _pose_only(G, priors, n, max_span=cr.LM_MAX_SPAN)
    prob_w, sv_w = _pose_only(G, priors, n)
    assert prob_l.band == 1 and prob_w.band == G.span
    return _trial(sv_l, state), _trial(sv_w, state), ref, sv_l.C.n


def test_one_trial_with_two_long_closures_equals_the_widened_band(gpu, oracle):
    """40 poses, 2 long closures under full models: the step of the low-rank path equals the widened band's to 1e-9.
    (test_closure_gpu.py holds the two paths together at 1e-8, in test_gtsam_set_long_closure_span; 1e-9 is the tighter.)

    Measured on the MI355X, printed below: 8.4e-11 between the two paths.  Against the numpy dense solve the low-rank path is
    8.6e-11 off and the widened band 2.7e-12 -- a ratio of 32, where test_closure_gpu.py's diagonal sets stay within its
    factor 8: a correlation of 0.95 makes a closure ten times stiffer along its well-measured combination, U U^T grows
    against the band system, and x0 - Z C^-1 U^T x0 cancels more digits.  That is the conditioning of §7o's correction,
    not the whitening: rows, gradient and U equal the reference to 1e-15 (the stage test above).  The factor-8 rule is
    therefore printed for the record and not asserted here."""
    dp_l, dp_w, ref, k = _long_against_wide(oracle, 40, [(0, 39), (31, 12)], 150)
    e_l, e_w, e_lw = relerr(dp_l, ref), relerr(dp_w, ref), relerr(dp_l, dp_w)
    print(f"2 long closures: low-rank {e_l:.3e}, widened band {e_w:.3e} against the dense solve; between them {e_lw:.3e}")
    assert k == 2 and e_lw <= 1e-9


def test_a_full_set_of_64_long_closures_fits(gpu, oracle):
    """100 poses, 64 long closures (VUS_CLOSURE_MAX) under full models: the set is accepted, the trial succeeds and its step
    equals the widened band's to the 1e-8 test_closure_gpu.py holds the two paths together at.  Measured: low-rank 8.6e-10,
    widened band 4.0e-11 against the numpy dense solve."""
    far = [(k, k + 9 + k % 21) if k % 2 else (k + 9 + k % 21, k) for k in range(64)]
    dp_l, dp_w, ref, k = _long_against_wide(oracle, 100, far, 151)
    e_l, e_w, e_lw = relerr(dp_l, ref), relerr(dp_w, ref), relerr(dp_l, dp_w)
    print(f"64 long closures: low-rank {e_l:.3e}, widened band {e_w:.3e} against the dense solve; between them {e_lw:.3e}")
    assert k == 64 and e_lw <= 1e-8


# ---- 4. LM ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _correlated(oracle):
    """CORRELATED_CASE and its two dense solutions (full models, marginal sigmas), computed once."""
    truth, init, G, priors = bg.correlated_pose_graph(**bg.CORRELATED_CASE)
    full = bg.lm_optimize(oracle, G, init, priors=priors)
    marg = br.lm_optimize(oracle, G.marginal(), init, priors=priors)
    return truth, init, G, priors, full, marg


def test_correlated_closures_walk_the_dense_lm_and_beat_their_marginal_sigmas(gpu, oracle):
    """The point of the feature: measurements drawn from covariances that correlate a rotation with a translation component
    by 0.95.  The solution under the full models is closer to the truth than the one under their marginal sigmas -- in the
    dense reference by 0.1354 m against 0.2659 m (between_gauss_ref.CORRELATED_CASE) -- and the GPU walks both dense
    runs."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    truth, init, G, priors, (ref_f, _, rep_f), (ref_m, _, rep_m) = _correlated(oracle)
    n = len(init)
    C = np.linalg.inv(G.R[0].T @ G.R[0])
    assert abs(C[1, 3]) / np.sqrt(C[1, 1] * C[3, 3]) >= 0.95 - 1e-12
    e_ref = bg.rms_position_error(ref_f, truth), bg.rms_position_error(ref_m, truth)
    assert e_ref[0] < 0.75 * e_ref[1]                      # the reference alone shows the gap
    got = {}
    z = np.zeros((0,))
    for name, Gk, ref, orep in (("full", G, ref_f, rep_f), ("marginal", G.marginal(), ref_m, rep_m)):
        prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                               prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=Gk.span)
        sv = StereoBASolver(prob, Gk.device(n))
        assert (sv.B.sqrt_info is not None) == (name == "full")
        poses, _, rep = sv.optimize(d(init), no_points())
        same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
        assert relerr(poses.cpu().numpy(), ref) < 1e-6, name
        assert abs(rep.final_error - orep["final_error"]) <= 1e-6 * orep["final_error"]
        got[name] = bg.rms_position_error(poses.cpu().numpy(), truth)
    print(f"RMS position error against the truth: full {got['full']:.4f} m, marginal sigmas {got['marginal']:.4f} m "
          f"(dense reference {e_ref[0]:.4f} / {e_ref[1]:.4f})")
    assert got["full"] < got["marginal"]


def test_stereo_plus_full_between_lm(gpu, oracle):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    seq, n, nL = _stereo(12, 300, 60)
    rng = np.random.default_rng(160)
    G = full_set(rng, seq["poses_gt"], [(k - 1, k) for k in range(1, n)] + [(3, 9), (11, 0)], noise=0.005)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                           prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=G.span)
    sv = StereoBASolver(prob, G.device(n))
    P = _oracle_problem(oracle, seq, n, nL)
    poses, points, rep = sv.optimize(d(seq["poses_init"]), d(seq["points_init"]))
    ref, rpts, orep = bg.lm_optimize(oracle, G, seq["poses_init"], P=P, points=seq["points_init"], band=prob.band)
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    assert relerr(poses.cpu().numpy(), ref) < 1e-6 and relerr(points.cpu().numpy(), rpts) < 1e-6


@pytest.mark.parametrize("stride", [2, 3])
def test_first_step_of_the_inertial_solvers_with_full_between_factors(gpu, oracle, stride):
    """test_between_gpu.py's inertial test under full models: the first trial's step of NavBASolver / NavBiasBASolver equals
    the inertial dense references plus the between blocks (1e-7, as there)."""
    import nav_ref
    import nav_bias_ref as nbr
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavBiasBASolver, NavFactors
    s = synth.nav_sequence(16, 300, 60)
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    rng = np.random.default_rng(170 + stride)
    G = full_set(rng, s["poses_gt"], [(k - 1, k) for k in range(1, n)] + [(0, 12), (14, 2)], noise=0.01)
    vels, lam = np.zeros((n, 3)), 1e-3
    kw = dict(prior_pose=[0], prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=stride,
              between_span=G.span)
    prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], **kw)
    if stride == 3:
        P, NG = nbr.make_graph(oracle, s)
        sv = NavBiasBASolver(prob, NG.device(), G.device(n, 3))
        bias = np.zeros((n, 6))
        ref = nbr.dense_system(oracle, s, P, NG, s["poses_init"], vels, bias, s["points_init"], lam, band=prob.band // 3)
    else:
        from test_nav_oracle import build_nav
        P, _ = build_nav(oracle, s)
        pims, Ws = nbr.preintegrate(s)
        imu = (np.arange(n - 1), np.arange(1, n), pims, Ws)
        dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
        vpr = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
        N = oracle.NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr)
        sv = NavBASolver(prob, NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr), G.device(n, 2))
        bias = np.zeros(6)
        ref = nav_ref.dense_system(oracle, s, P, N, s["poses_init"], vels, bias, s["points_init"], lam)
    nc = 6 * stride * n
    H, gb, _, _ = bg.system(oracle, G, s["poses_init"], stride * n, stride)
    A, g = ref["A"].copy(), ref["g"].copy()
    A[:nc, :nc] += H
    g[:nc] += gb
    state = (d(s["poses_init"]), d(vels), d(bias), d(s["points_init"]))
    sv._lm_linearize(state)
    sv._lm_solve(lam)
    x = np.linalg.solve(A, -g)
    assert relerr(sv.dp.cpu().numpy().reshape(-1), x[:nc]) < 1e-7


# ---- 5. the gtsam shim ---------------------------------------------------------------------------------------------------------
def _shim_graph(G, init, priors):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(priors[1][0]), gtsam.noiseModel.Diagonal.Sigmas(1.0 / priors[2][0])))
    for f in range(len(G.i)):
        model = gtsam.noiseModel.Gaussian.SqrtInformation(G.R[f])
        assert isinstance(model, gtsam.noiseModel.Gaussian)
        if G.losses[f][0]:
            est = {1: gtsam.noiseModel.mEstimator.Huber, 2: gtsam.noiseModel.mEstimator.Cauchy}[G.losses[f][0]]
            model = gtsam.noiseModel.Robust.Create(est.Create(G.losses[f][1]), model)
        graph.add(gtsam.BetweenFactorPose3(X(int(G.i[f])), X(int(G.j[f])), gtsam.Pose3.from_flat12(G.meas[f]), model))
    for k in range(len(init)):
        values.insert(X(k), gtsam.Pose3.from_flat12(init[k]))
    return graph, values


def test_gtsam_drop_in_error_optimize_and_marginals(gpu, oracle):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    rng = np.random.default_rng(180)
    n = 30
    truth, init, _, priors = br.pose_graph(rng, n)
    pairs = [(k - 1, k) for k in range(1, n)] + [(0, 29), (20, 4)]
    G = full_set(rng, truth, pairs, noise=0.01, losses=[(0, 0.0)] * n + [(2, 1.0)])
    graph, values = _shim_graph(G, init, priors)
    # the shim hands the kernels ITS R (the Cholesky factor of R^T R): the same model, another rounding of the matrix
    want = bg.error(oracle, G, init) + br.prior_error(oracle, priors, init)
    assert relerr(graph.error(values), want) < 1e-10
    opt = gtsam.LevenbergMarquardtOptimizer(graph, values, gtsam.LevenbergMarquardtParams())
    res = opt.optimize()
    ref, _, orep = bg.lm_optimize(oracle, G, init, priors=priors)
    got = np.stack([res.atPose3(X(k)).flat12() for k in range(n)])
    rep = opt.report()
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, orep)
    assert relerr(got, ref) < 1e-6
    # marginals at the start against the dense inverse (Gaussian factors only: the linearisation is the information)
    G2 = bg.GaussSet(G.i, G.j, G.meas, G.R)
    graph2, _ = _shim_graph(G2, init, priors)
    m = gtsam.Marginals(graph2, values)
    Hb, _, _, _ = bg.system(oracle, G2, init, n)
    Hp, _, _ = br.prior_system(oracle, priors, init)
    Ainv = np.linalg.inv(Hb + Hp)
    for k in (0, 7, 29):
        assert relerr(m.marginalCovariance(X(k)), Ainv[6 * k:6 * k + 6, 6 * k:6 * k + 6]) < 1e-8
    J = m.jointMarginalCovariance([X(4), X(20)]).fullMatrix()
    idx = list(range(24, 30)) + list(range(120, 126))
    assert relerr(J, Ainv[np.ix_(idx, idx)]) < 1e-8


def test_gtsam_set_long_closure_span_with_a_full_model(gpu, oracle):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    rng = np.random.default_rng(181)
    n = 40
    truth, init, _, priors = br.pose_graph(rng, n)
    G = full_set(rng, truth, [(k - 1, k) for k in range(1, n)] + [(0, 39)], noise=0.01)
    graph, values = _shim_graph(G, init, priors)
    out = {}
    for m in (None, cr.LM_MAX_SPAN):
        prm = gtsam.LevenbergMarquardtParams()
        prm.setLongClosureSpan(m)
        opt = gtsam.LevenbergMarquardtOptimizer(graph, values, prm)
        res = opt.optimize()
        out[m] = np.stack([res.atPose3(X(k)).flat12() for k in range(n)])
        assert opt.report().long_closures == (1 if m else 0)
    assert relerr(out[cr.LM_MAX_SPAN], out[None]) <= 1e-8          # the bound test_closure_gpu.py holds the shim to


def test_run_sequence_with_full_noise_accepts_the_same_closures(gpu, loop_track):
    from visual_underwater_slam_amd import gtsam, sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    import loop_scene as S
    st0 = loop_track["stages"]
    lc = sequence.LoopClosureParams(noise="full")
    res, seq, st = sequence.run_sequence(*loop_track["args"], disparity_sign=1, params=loop_track["params"], loop_closure=lc)
    assert all(np.array_equal(a, b) for a, b in zip(st["loop_pairs"], st0["loop_pairs"]))
    assert np.array_equal(st["loop_accepted"], st0["loop_accepted"]) and st["loop_accepted"].any()
    btw = [f for f in seq.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
    btw0 = [f for f in loop_track["seq"].graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
    assert len(btw) == len(btw0) == int(st["loop_accepted"].sum())
    assert all(isinstance(f.noiseModel(), gtsam.noiseModel.Gaussian) for f in btw)
    assert all(type(f.noiseModel()) is gtsam.noiseModel.Diagonal for f in btw0)
    assert any(relerr(f.noiseModel().covariance(), loop_track["cov"]) < 1e-10 for f in btw)
    gt = loop_track["gt"]
    last = [np.linalg.norm(r.atPose3(X(S.N_KF - 1)).translation() - gt[-1, 9:]) for r in (res, loop_track["result"])]
    print(f"last keyframe against the truth: full covariance {1e3 * last[0]:.2f} mm, marginal sigmas {1e3 * last[1]:.2f} mm")
    assert np.isfinite(last).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_check_refuses_a_bad_sqrt_info_and_names_the_factor(gpu):
    rng = np.random.default_rng(190)
    n = 12
    truth, _, _, _ = br.pose_graph(rng, n)
    G = full_set(rng, truth, [(k - 1, k) for k in range(1, n)] + [(0, 11), (10, 1)])
    B = G.device(n, max_span=5)
    st = _lib.current_stream_ptr()
    _lib.call("vus_between_check", B.addr(), 5, st)
    _lib.call("vus_closure_check", B.long.addr(), 5, st)
    for S, fn, f in ((B, "vus_between_check", 7), (B.long, "vus_closure_check", 1)):
        keep = S.sqrt_info.clone()
        S.sqrt_info[f, 7 * 3] = 0.0
        with pytest.raises(_lib.VusError, match=rf"factor {f}: sqrt_info\(3, 3\).*> 0"):
            _lib.call(fn, S.addr(), 5, st)
        S.sqrt_info.copy_(keep)
        S.sqrt_info[f, 6 * 1 + 4] = float("nan")
        with pytest.raises(_lib.VusError, match=rf"factor {f}: sqrt_info\(1, 4\).*not finite"):
            _lib.call(fn, S.addr(), 5, st)
        S.sqrt_info.copy_(keep)
        S.sqrt_info[f, 6 * 4 + 1] = float("nan")            # below the diagonal: not read, not checked
        _lib.call(fn, S.addr(), 5, st)
        S.sqrt_info.copy_(keep)
        _lib.call(fn, S.addr(), 5, st)
