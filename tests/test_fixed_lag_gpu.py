"""Fixed-lag smoothing on the MI355X (include/vus_fixed_lag.h, ba.WindowPrior, StereoBASolver.marginalize_head) against the
dense f64 statement of fixed_lag_ref.py.

Tolerances: the family stages are kernels, 1e-11 relative (the kernel class of lm_ref.tolerance).  What sits behind an
inverse is held to 100 x the discrepancy measured between two CPU evaluations of the reference that sum in different orders
(Cholesky of S_MM and all of M at once, against np.linalg.solve and one node at a time), never tighter than the 1e-8 of the
after-a-solve class: the rule of lm_ref.tolerance, for its reason -- the GPU sums in a third order."""
import numpy as np
import pytest
import torch

import between_ref as br
import fixed_lag_ref as fl
import marginals_ref as mr
from visual_underwater_slam_amd import synth, _lib

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-11


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def solve_tol(floor):
    return max(100.0 * floor, 1e-8)


# -- 1. the family stages ------------------------------------------------------------------------------------------------
def _pose_only_solver(n, band, priors, G=None, window=None):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    z = np.zeros((0,))
    prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                           prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=band)
    return prob, StereoBASolver(prob, None if G is None else G.device(n), window_prior=window)


def _window(rng, truth, first, m, n, singular=False):
    from visual_underwater_slam_amd.ba import WindowPrior
    M = rng.normal(size=(6 * m, 6 * m + 3))
    H = M @ M.T
    if singular:                                    # a gauge direction: H v = 0
        v = rng.normal(size=6 * m)
        Pm = np.eye(6 * m) - np.outer(v, v) / (v @ v)
        H = Pm @ H @ Pm
        H = 0.5 * (H + H.T)
    ref = fl.Prior(first, truth[first:first + m].copy(), H, rng.normal(size=6 * m), 0.37)
    return ref, WindowPrior(first, ref.x0, ref.H, ref.g, ref.c, n)


@pytest.mark.parametrize("m", [1, 2, 9])
@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("wide", [False, True])
def test_stages_against_the_reference(gpu, oracle, m, at_end, wide):
    n = 14
    rng = np.random.default_rng(100 * m + 10 * at_end + wide)
    truth, _, _, priors = br.pose_graph(rng, n)
    # displaced from x0 by rotations up to ~0.3 rad: delta != 0
    init = np.stack([oracle.pose_retract(T, np.r_[0.17 * rng.uniform(-1, 1, 3), 0.2 * rng.normal(size=3)]) for T in truth])
    first, band = (n - m if at_end else 0), (12 if wide else m - 1)
    ref, W = _window(rng, truth, first, m, n, singular=(m == 2))
    prob, sv = _pose_only_solver(n, band, priors, window=W)
    assert prob.band == band and len(sv._trial) == 5 + 4
    assert np.abs(fl.delta(oracle, ref, init)).max() > 0.05
    poses, points = d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    Href, gref, eref = fl.system(oracle, ref, init, n)
    assert relerr(sv.window_prior_error(poses), eref) < STAGE_TOL
    sv.linearize(poses, points)
    sv.window_prior_linearize(poses)
    assert relerr(sv.wp_scal[0].item(), eref) < STAGE_TOL
    s = slice(6 * first, 6 * (first + m))
    assert relerr(sv.wp_grad.cpu().numpy(), gref[s]) < STAGE_TOL
    # assemble on top of a Schur result, twice: bit-identical
    sv.Sband.zero_()
    sv.schur(1e-3)
    S0, g0 = sv.Sband.clone(), sv.gs.clone()
    runs = []
    for _ in range(2):
        sv.Sband.copy_(S0)
        sv.gs.copy_(g0)
        sv.window_prior_assemble()
        runs.append((sv.Sband.cpu().numpy().copy(), sv.gs.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    want = S0.cpu().numpy() + mr.dense_to_band(Href, band).reshape(n, band + 1, 36)
    assert relerr(runs[0][0], want) < STAGE_TOL
    assert relerr(runs[0][1].reshape(-1), g0.cpu().numpy().reshape(-1) + gref) < STAGE_TOL
    # a step: the linearised error at the old poses, the error at the retracted ones
    x = 0.02 * rng.normal(size=6 * n)
    new = np.stack([oracle.pose_retract(init[k], x[6 * k:6 * k + 6]) for k in range(n)])
    sv.dp.copy_(d(x.reshape(n, 6)))
    sv.new_poses.copy_(d(new))
    sv.window_prior_eval_step(poses)
    out = sv.wp_scal.cpu().numpy()
    assert relerr(out[1], fl.linear_error(oracle, ref, init, x)) < STAGE_TOL
    assert relerr(out[2], fl.error(oracle, ref, new)) < STAGE_TOL


def test_without_the_family_nothing_is_added(gpu):
    rng = np.random.default_rng(5)
    _, _, _, priors = br.pose_graph(rng, 6)
    _, sv = _pose_only_solver(6, 2, priors)
    assert len(sv._trial) == 5 and "window_prior" not in sv._families and not hasattr(sv, "wp_grad")
    assert sv.window_prior_error(None) == 0.0


def test_the_check_refuses_a_bad_hessian_by_name(gpu):
    from visual_underwater_slam_amd.ba import WindowPrior
    n, m = 6, 2
    rng = np.random.default_rng(6)
    truth, _, _, priors = br.pose_graph(rng, n)
    M = rng.normal(size=(6 * m, 6 * m))
    H = M @ M.T

    def build(Hx, g=None, c=0.0):
        W = WindowPrior(1, truth[1:1 + m], Hx, np.zeros(6 * m) if g is None else g, c, n)
        return _pose_only_solver(n, 3, priors, window=W)
    build(H)
    Z = H.copy()
    Z[4], Z[:, 4] = 0.0, 0.0                          # positive semi-definite with a free direction: accepted
    build(Z)
    A = H.copy()
    A[2, 7] += 1e-6 * np.abs(H).max()
    bad = H.copy()
    bad[3, 3] = float("nan")
    neg = H.copy()
    neg[5, 5] = -1e-3
    for Hx, kw, word in ((A, {}, "not symmetric"), (bad, {}, "not finite"), (neg, {}, "negative diagonal"),
                         (H, dict(g=np.r_[np.inf, np.zeros(6 * m - 1)]), "not finite"), (H, dict(c=float("inf")), "not finite")):
        with pytest.raises(_lib.VusError, match=word):
            build(Hx, **kw)


# -- 2. vus_ba_band_marginalize alone -----------------------------------------------------------------------------------
def _marginalize(Sb, gs, n, band, k):
    w = n - k
    H = torch.full((6 * w, 6 * w), float("nan"), dtype=torch.float64, device="cuda")
    g = torch.full((6 * w,), float("nan"), dtype=torch.float64, device="cuda")
    quad = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().vus_ba_band_marginalize_work_doubles(n, band, k)), dtype=torch.float64, device="cuda")
    assert work.numel() > 0
    Sd, gd = d(Sb), d(gs)
    p = _lib.ptr
    _lib.call("vus_ba_band_marginalize", p(Sd), n, band, p(gd), k, p(H), p(g), p(quad), p(status), p(work), _lib.current_stream_ptr())
    return H.cpu().numpy(), g.cpu().numpy(), float(quad.item()), int(status.item())


_CASES = sorted({(band, k, w) for band in (1, 3, 12) for k in (1, 7, 8, 9) for w in (1, band, band + 1) if band < k + w})


@pytest.mark.parametrize("band,k,w", _CASES)
def test_band_marginalize_against_the_dense_schur_complement(gpu, band, k, w):
    n = k + w
    rng = np.random.default_rng(1000 * band + 10 * k + w)
    A, Sb = mr.random_spd_band(rng, n, band)
    b = rng.normal(size=6 * n) * np.abs(A).max()
    Href, gref, cref = fl.marginal_head(A, b, 0.0, k)
    H2, g2, c2 = fl.marginal_head(A, b, 0.0, k, one_at_a_time=True, solve="lu")
    floor = max(relerr(H2, Href), relerr(g2, gref), abs(c2 - cref) / abs(cref))
    tol = solve_tol(floor)
    H, g, quad, status = _marginalize(Sb, b.reshape(n, 6), n, band, k)
    print(f"band={band} n_drop={k} w={w}: floor {floor:.2e}, H {relerr(H, Href):.2e}, g {relerr(g, gref):.2e}, "
          f"quad {abs(-0.5 * quad - cref) / abs(cref):.2e}")
    assert status == 0
    assert np.array_equal(H, H.T)                    # both triangles, mirrored
    assert relerr(H, Href) < tol and relerr(g, gref) < tol and abs(-0.5 * quad - cref) < tol * abs(cref)
    again = _marginalize(Sb, b.reshape(n, 6), n, band, k)
    assert np.array_equal(H, again[0]) and np.array_equal(g, again[1]) and quad == again[2]


@pytest.mark.parametrize("row", [0, 5, 47, 50])
def test_band_marginalize_names_the_first_non_positive_pivot(gpu, row):
    band, k, w = 3, 9, 4
    n = k + w
    rng = np.random.default_rng(row)
    A, _ = mr.random_spd_band(rng, n, band)
    L = np.linalg.cholesky(A[:6 * k, :6 * k])
    A[row, row] -= L[row, row] ** 2 * 1.5            # the pivot of this row becomes negative, the rows before it are untouched
    *_, status = _marginalize(mr.dense_to_band(A, band), rng.normal(size=(n, 6)), n, band, k)
    assert status == 1 + row


def test_a_dropped_pose_without_information_is_named(gpu):
    from visual_underwater_slam_amd.ba import IndeterminantSystem
    band, k, w = 3, 4, 3
    n = k + w
    rng = np.random.default_rng(9)
    A, _ = mr.random_spd_band(rng, n, band)
    A[12:18], A[:, 12:18] = 0.0, 0.0                 # node 2 carries nothing
    *_, status = _marginalize(mr.dense_to_band(A, band), rng.normal(size=(n, 6)), n, band, k)
    assert (status - 1) // 6 == 2
    # through the solver: pose 0 of a graph whose only factors are a prior on pose 2 and odometry 1 - 2
    truth, init, _, _ = br.pose_graph(rng, 3)
    G = br.BetweenSet([1], [2], [br.flat_mul(br.flat_inv(truth[1]), truth[2])], [[0.01] * 3 + [0.05] * 3])
    priors = (np.array([2]), truth[2:3], np.array([[1e2] * 6]))
    _, sv = _pose_only_solver(3, 2, priors, G)
    with pytest.raises(IndeterminantSystem) as e:
        sv.marginalize_head(d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"), 1)
    assert (e.value.kind, e.value.index) == ("node", 0)
    with pytest.raises(ValueError, match="n_drop"):
        sv.marginalize_head(d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"), 3)


# -- 3. marginalisation is exact at the linearisation point -----------------------------------------------------------
N_KF = 12


@pytest.fixture(scope="module")
def scene():
    """12 keyframes on one line over ~150 landmarks, odometry between factors and one in-band closure (1, 5)."""
    from visual_underwater_slam_amd.gtsam import Pose3
    seq = synth.ba_sequence(N_KF, 260, 40, line_len=N_KF)
    rng = np.random.default_rng(11)
    pairs = [(k - 1, k) for k in range(1, N_KF)] + [(1, 5)]
    meas = [Pose3.from_flat12(seq["poses_gt"][a]).between(Pose3.from_flat12(seq["poses_gt"][b])).retract(
        0.01 * rng.standard_normal(6)).flat12() for a, b in pairs]
    G = br.BetweenSet([p[0] for p in pairs], [p[1] for p in pairs], np.array(meas), np.tile([0.01] * 3 + [0.05] * 3, (len(pairs), 1)))
    assert 100 <= len(seq["points_gt"]) <= 400
    return seq, G


def _sub_solver(seq, G, pose0, n, lm_ids, obs_mask, btw_mask, prior0, loss, span, window=None):
    """The solver of a part of the scene: poses pose0 .. pose0 + n - 1, the landmarks lm_ids, the observations and between
    factors the masks select, the prior on pose 0 if asked; everything re-indexed."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    lm_map = -np.ones(len(seq["points_gt"]), np.int64)
    lm_map[lm_ids] = np.arange(len(lm_ids))
    op, ol = seq["obs_pose"][obs_mask] - pose0, lm_map[seq["obs_point"][obs_mask]]
    assert (op >= 0).all() and (op < n).all() and (ol >= 0).all()
    kw = dict(prior_pose=[0], prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None]) if prior0 else {}
    prob = StereoBAProblem(op.astype(np.int32), ol.astype(np.int32), seq["meas"][obs_mask], n, len(lm_ids), seq["K"], seq["sigma"],
                           between_span=span, loss=loss, **kw)
    Gs = None
    if btw_mask.any():
        Gs = br.BetweenSet(G.i[btw_mask] - pose0, G.j[btw_mask] - pose0, G.meas[btw_mask], 1.0 / G.w[btw_mask])
    return prob, StereoBASolver(prob, None if Gs is None else Gs.device(n), window_prior=window), Gs


def _undamped_step(sv, poses, points):
    sv._linearize_all((poses, points))
    sv._assemble_zero()
    sv.band_solve()
    sv.backsub()
    assert int(sv.status.item()) == 0
    return sv.dp.cpu().numpy().copy(), sv.dl.cpu().numpy().copy()


def _dense(oracle, sv, Gs, poses_np, extra=None):
    """Dense (A, b, e0) over [poses, landmarks] of a solver's graph at its last linearisation: the stereo products the GPU
    left (robust weights included), the between factors and an optional pose-side system by their numpy statements."""
    lin = {k: getattr(sv, k).cpu().numpy() for k in ("W", "V", "gl", "Hpp", "gp")}
    pk = sv.P.pk
    A, b = fl.full_dense(lin, pk["obs_pose"].cpu().numpy(), pk["obs_point"].cpu().numpy(), sv.P.n_poses, sv.P.n_points)
    e0 = float(sv.scal[0].item())
    for Hx, gx, ex in ([br.system(oracle, Gs, poses_np, sv.P.n_poses)[:3]] if Gs is not None else []) + ([extra] if extra else []):
        A, b = fl.add_poses(A, b, Hx, gx)
        e0 += ex
    return A, b, e0


@pytest.mark.parametrize("loss", [None, ("huber", 1.0)], ids=["gaussian", "huber"])
@pytest.mark.parametrize("k", [1, 3])
def test_marginalisation_is_exact_at_the_linearisation_point(gpu, oracle, scene, loss, k):
    from visual_underwater_slam_amd.ba import WindowPrior
    seq, G = scene
    n, nL = N_KF, len(seq["points_gt"])
    op, ol = seq["obs_pose"], seq["obs_point"]
    every = np.ones(len(op), bool)
    poses_np, points_np = seq["poses_init"], seq["points_init"]
    # the full graph
    _, full, _ = _sub_solver(seq, G, 0, n, np.arange(nL), every, np.ones(len(G.i), bool), True, loss, G.span)
    dp_full, dl_full = _undamped_step(full, d(poses_np), d(points_np))
    A, b, e0 = _dense(oracle, full, G, poses_np)
    cov_full = full.marginals(d(poses_np), d(points_np), points_cov=False).pose_cov.cpu().numpy()
    # the absorbed set: every landmark an expired pose sees with all its observations, the prior on pose 0, every
    # between factor that touches an expired pose
    gone = np.zeros(nL, bool)
    gone[ol[op < k]] = True
    obs_A = gone[ol]
    btw_A = (G.i < k) | (G.j < k)
    touched = np.r_[op[obs_A], G.i[btw_A], G.j[btw_A]]
    nA = int(touched.max()) + 1
    assert set(range(nA)) <= set(touched.tolist()) and k < nA < n
    lm_A, lm_R = np.nonzero(gone)[0], np.nonzero(~gone)[0]
    assert len(lm_A) and len(lm_R)
    _, svA, GA = _sub_solver(seq, G, 0, nA, lm_A, obs_A, btw_A, True, loss, nA - 1)
    W = svA.marginalize_head(d(poses_np[:nA]), d(points_np[lm_A]), k)
    assert (W.first, W.m, W.n_poses) == (0, nA - k, nA - k) and torch.equal(W.x0, d(poses_np[k:nA]))
    # the same by the dense statement, and the floor between its two orders of summation
    AA, bA, eA = _dense(oracle, svA, GA, poses_np[:nA])
    Href, gref, cref = fl.marginal(AA, bA, eA, list(range(6 * k)) + list(range(6 * nA, len(bA))))
    H2, g2, c2 = fl.marginal_head(*fl.marginal(AA, bA, eA, range(6 * nA, len(bA)), "lu"), k, one_at_a_time=True, solve="lu")
    tolA = solve_tol(max(relerr(H2, Href), relerr(g2, gref), abs(c2 - cref) / abs(cref)))
    got = (W.H.cpu().numpy(), W.g.cpu().numpy(), W.c_const)
    print(f"k={k} loss={loss}: prior H {relerr(got[0], Href):.2e} g {relerr(got[1], gref):.2e} c {abs(got[2] - cref) / abs(cref):.2e} tol {tolA:.2e}")
    assert relerr(got[0], Href) < tolA and relerr(got[1], gref) < tolA and abs(got[2] - cref) < tolA * abs(cref)
    # the reduced graph: the rest + the prior
    nR = n - k
    Wr = WindowPrior(0, W.x0, W.H, W.g, W.c_const, nR)
    _, red, GR = _sub_solver(seq, G, k, nR, lm_R, ~obs_A, ~btw_A, False, loss, nR - 1, window=Wr)
    dp_red, dl_red = _undamped_step(red, d(poses_np[k:]), d(points_np[lm_R]))
    # floor: the full dense system solved directly against marginalised first, both on the CPU
    elim = list(range(6 * k)) + [6 * n + 3 * int(j) + c for j in lm_A for c in range(3)]
    keep = np.setdiff1d(np.arange(len(b)), elim)
    x_full = np.linalg.solve(A, -b)
    Hm, gm, _ = fl.marginal(A, b, e0, elim)
    x_red = np.linalg.solve(Hm, -gm)
    tol = solve_tol(relerr(x_red, x_full[keep]))
    print(f"  step: poses {relerr(dp_red, dp_full[k:]):.2e} landmarks {relerr(dl_red, dl_full[lm_R]):.2e} tol {tol:.2e}")
    assert relerr(dp_red, dp_full[k:]) < tol and relerr(dl_red, dl_full[lm_R]) < tol
    assert relerr(dp_full.reshape(-1), x_full[:6 * n]) < tol                 # and the GPU's full step is the dense one
    cov_red = red.marginals(d(poses_np[k:]), d(points_np[lm_R]), points_cov=False).pose_cov.cpu().numpy()
    cov_ref = np.linalg.inv(Hm)
    tol_cov = solve_tol(relerr(np.linalg.inv(A)[np.ix_(keep, keep)][:6 * nR, :6 * nR], cov_ref[:6 * nR, :6 * nR]))
    print(f"  pose_cov {relerr(cov_red, cov_full[k:]):.2e} tol {tol_cov:.2e}")
    assert relerr(cov_red, cov_full[k:]) < tol_cov
    # prior on prior: the kept poses displaced (delta != 0), the head of the reduced graph marginalised again -- against the
    # numpy statement doing the same two steps from its own first prior
    moved = np.stack([oracle.pose_retract(T, 0.01 * np.random.default_rng(3).standard_normal(6)) for T in poses_np[k:]])
    W2 = red.marginalize_head(d(moved), d(points_np[lm_R]), 1)
    prior1 = fl.Prior(0, poses_np[k:nA].copy(), Href, gref, cref)
    assert np.abs(fl.delta(oracle, prior1, moved)).max() > 1e-3
    AR, bR, eR = _dense(oracle, red, GR, moved, extra=fl.system(oracle, prior1, moved, nR))
    H3, g3, c3 = fl.marginal(AR, bR, eR, list(range(6)) + list(range(6 * nR, len(bR))))
    H4, g4, c4 = fl.marginal_head(*fl.marginal(AR, bR, eR, range(6 * nR, len(bR)), "lu"), 1, one_at_a_time=True, solve="lu")
    tol2 = solve_tol(max(relerr(H4, H3), relerr(g4, g3), abs(c4 - c3) / abs(c3), tolA / 100.0))
    got = (W2.H.cpu().numpy(), W2.g.cpu().numpy(), W2.c_const)
    print(f"  prior on prior: H {relerr(got[0], H3):.2e} g {relerr(got[1], g3):.2e} c {abs(got[2] - c3) / abs(c3):.2e} tol {tol2:.2e}")
    assert W2.m == nR - 1
    assert relerr(got[0], H3) < tol2 and relerr(got[1], g3) < tol2 and abs(got[2] - c3) < tol2 * abs(c3)


# -- 4. the smoother end to end -----------------------------------------------------------------------------------------
def test_the_smoother_follows_the_full_batch(gpu):
    """24 keyframes of a stereo track with odometry, noise drawn at the sigmas the noise models state, lag = 8 keyframes,
    one keyframe per update.  The newest pose of the smoother lies within ONE standard deviation of its own batch marginal
    of the full-batch optimum: a consistent smoother differs from the batch only by the linearisation error of what it
    absorbed, small against the posterior spread; a sign error in g or a double-counted or dropped prior is not.  The same
    difference for a window that drops old factors with no prior and pins its first pose is printed, not asserted
    (profiles/fixed_lag.md keeps both)."""
    from visual_underwater_slam_amd import gtsam, gtsam_unstable
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    n, lag = 24, 8.0
    seq = synth.ba_sequence(n, 400, 30, line_len=n, meas_sigma=1.0)
    assert len(seq["points_gt"]) <= 400
    rng = np.random.default_rng(4)
    K = gtsam.Cal3_S2Stereo(*seq["K"])
    stereo_noise = gtsam.noiseModel.Isotropic.Sigma(3, 1.0)
    odo_sig = np.array([0.005] * 3 + [0.02] * 3)
    odo_noise = gtsam.noiseModel.Diagonal.Sigmas(odo_sig)
    prior_noise = gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])
    gt = [gtsam.Pose3.from_flat12(T) for T in seq["poses_gt"]]
    odo = [gt[i - 1].between(gt[i]).retract(odo_sig * rng.standard_normal(6)) for i in range(1, n)]
    obs_of = [np.nonzero(seq["obs_pose"] == i)[0] for i in range(n)]

    def pose_factors(i):
        if i == 0:
            return [gtsam.PriorFactorPose3(X(0), gt[0], prior_noise)]
        return [gtsam.BetweenFactorPose3(X(i - 1), X(i), odo[i - 1], odo_noise)]

    def stereo(i, rows):
        return [gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*seq["meas"][a]), stereo_noise, X(i), L(int(seq["obs_point"][a])), K)
                for a in rows]

    # the full batch
    graph, init = gtsam.NonlinearFactorGraph(), gtsam.Values()
    pose = gt[0]
    for i in range(n):
        pose = pose.compose(odo[i - 1]) if i else gt[0]
        init.insert(X(i), pose)
        for f in pose_factors(i) + stereo(i, obs_of[i]):
            graph.push_back(f)
    for j in range(len(seq["points_gt"])):
        init.insert(L(j), seq["points_init"][j])
    batch = gtsam.LevenbergMarquardtOptimizer(graph, init, gtsam.LevenbergMarquardtParams()).optimize()
    cov = gtsam.Marginals(graph, batch).marginalCovariance(X(n - 1))
    one_sigma = float(np.sqrt(np.trace(cov[3:, 3:])))
    want = batch.atPose3(X(n - 1)).translation()

    # the smoother, and the bookkeeping of the rule from the visibility table
    sm = gtsam_unstable.BatchFixedLagSmoother(lag)
    present, live, ts = set(), set(), {}
    seen_cases = dict(marginalised=0, discarded=0, waiting=0)
    for i in range(n):
        g, theta, stamps = gtsam.NonlinearFactorGraph(), gtsam.Values(), {X(i): float(i)}
        for f in pose_factors(i) + stereo(i, obs_of[i]):
            g.push_back(f)
        theta.insert(X(i), sm.calculateEstimatePose3(X(i - 1)).compose(odo[i - 1]) if i else gt[0])
        ts[("x", i)] = float(i)
        for a in obs_of[i]:
            j = int(seq["obs_point"][a])
            if j not in present:        # new, or dropped earlier: a fresh value.  Three kinds of landmark timestamp:
                present.add(j)          # the first sighting, the latest sighting (below), three keyframes before the first
                theta.insert(L(j), seq["points_init"][j])
                ts[j] = float(i) - (3.0 if j % 3 == 2 else 0.0)
                stamps[L(j)] = ts[j]
            elif j % 3 == 1:
                ts[j] = float(i)
                stamps[L(j)] = ts[j]
            live.add((i, j))
        stats = sm.update(g, theta, stamps)
        cut = float(i) - lag
        expired = {p for p in range(i + 1) if ("x", p) in ts and ts[("x", p)] < cut}
        seen = {j for p, j in live if p in expired}
        gone = {j for j in seen if ts[j] < cut}
        discarded = {(p, j) for p, j in live if p in expired and j not in gone}
        seen_cases["waiting"] += len({j for p, j in live if ts[j] < cut} - seen)
        seen_cases["marginalised"] += len(gone)
        seen_cases["discarded"] += len(discarded)
        assert (stats["expired_poses"], stats["marginalized_landmarks"], stats["discarded_factors"]) == \
            (len(expired), len(gone), len(discarded)), i
        live = {(p, j) for p, j in live if p not in expired and j not in gone}
        present -= gone
        for p in expired:
            del ts[("x", p)]
        est = sm.calculateEstimate()
        n_window = len(est._pose3_table()[0])
        assert n_window == min(i + 1, int(lag) + 1) and n_window <= lag + 1
        assert all(not est.exists(L(j)) for j in gone) and all(not est.exists(X(p)) for p in expired)
        assert sum(isinstance(f, gtsam.LinearContainerFactor) for f in sm.getFactors()._factors) == int(i > lag)
    assert min(seen_cases.values()) > 0, seen_cases          # all three landmark cases occurred
    diff = float(np.linalg.norm(sm.calculateEstimatePose3(X(n - 1)).translation() - want))

    # recorded, not asserted: the same window with the old factors dropped and no prior, its first pose pinned
    pin = gtsam.noiseModel.Isotropic.Sigma(6, 1e-4)
    est = gtsam.Values()
    for i in range(n):
        lo = max(0, i - int(lag))
        g = gtsam.NonlinearFactorGraph()
        est.insert(X(i), est.atPose3(X(i - 1)).compose(odo[i - 1]) if i else gt[0])
        for a in obs_of[i]:
            if not est.exists(L(int(seq["obs_point"][a]))):
                est.insert(L(int(seq["obs_point"][a])), seq["points_init"][int(seq["obs_point"][a])])
        vals = gtsam.Values()
        for p in range(lo, i + 1):
            vals.insert(X(p), est.atPose3(X(p)))
            for f in (pose_factors(p) if p > lo else []) + stereo(p, obs_of[p]):
                g.push_back(f)
            for a in obs_of[p]:
                if not vals.exists(L(int(seq["obs_point"][a]))):
                    vals.insert(L(int(seq["obs_point"][a])), est.atPoint3(L(int(seq["obs_point"][a]))))
        g.push_back(gtsam.PriorFactorPose3(X(lo), est.atPose3(X(lo)), pin))
        res = gtsam.LevenbergMarquardtOptimizer(g, vals, gtsam.LevenbergMarquardtParams()).optimize()
        for k in vals.keys():
            est.update(k, res._at(k, object, "at"))
    diff_pinned = float(np.linalg.norm(est.atPose3(X(n - 1)).translation() - want))
    print(f"newest pose against the batch: smoother {diff:.4e} m = {diff / one_sigma:.3f} sigma, pinned window without a prior "
          f"{diff_pinned:.4e} m = {diff_pinned / one_sigma:.3f} sigma (one sigma = {one_sigma:.4e} m); cases {seen_cases}")
    assert diff <= one_sigma
