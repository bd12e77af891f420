"""The fixed-lag prior of an inertial window on the MI355X (include/vus_fixed_lag_nav.h, ba.NavWindowPrior,
NavBiasBASolver.marginalize_head) against the dense f64 statement of fixed_lag_nav_ref.py.

Tolerances are those of test_fixed_lag_gpu.py: the family stages are kernels, 1e-11 relative; what sits behind an inverse is
held to 100 x the discrepancy measured between two CPU evaluations of the reference that sum in different orders, never
tighter than 1e-8."""
import numpy as np
import pytest
import torch

import fixed_lag_nav_ref as fn
import fixed_lag_ref as fl
import marginals_ref as mr
import nav_bias_ref as nbr
from visual_underwater_slam_amd import synth, _lib

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-11
WALK = (2e-3, 2e-4)


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def solve_tol(floor):
    return max(100.0 * floor, 1e-8)


def _scene(n, n_lm, track, obs_per_kf=40):
    """A nav_sequence with a drifting bias whose landmarks are each kept for `track` + 1 consecutive keyframes from their
    first sighting, so that the landmark band stays narrow and a dropped keyframe's landmarks end inside the graph."""
    s = dict(synth.nav_sequence(n, n_lm, obs_per_kf, bias_walk_sigma=WALK))
    op, ol = s["obs_pose"], s["obs_point"]
    first = np.full(len(s["points_gt"]), n, np.int64)
    np.minimum.at(first, ol, op)
    keep = op - first[ol] <= track
    s["obs_pose"], s["obs_point"], s["meas"] = op[keep], ol[keep], s["meas"][keep]
    return s


def _displaced(oracle, rng, s):
    n = len(s["poses_gt"])
    poses = np.stack([oracle.pose_retract(T, np.r_[0.1 * rng.uniform(-1, 1, 3), 0.1 * rng.normal(size=3)]) for T in s["poses_gt"]])
    return poses, s["vels_gt"] + 0.05 * rng.normal(size=(n, 3)), s["biases_gt"] + 0.01 * rng.normal(size=(n, 6))


def _device_prior(W, n):
    from visual_underwater_slam_amd.ba import NavWindowPrior
    return NavWindowPrior(W.first, W.x0, W.v0, W.b0, W.H, W.g, W.c, n)


def _solver(s, G, window=None, band=None, span=0, loss=None, prior0=True, n=None, obs=None, n_points=None):
    """The GPU problem (pose_stride 3) and NavBiasBASolver of a graph; `obs` = (obs_pose, obs_point, meas) of a part."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBiasBASolver
    n = len(s["poses_gt"]) if n is None else n
    op, ol, meas = (s["obs_pose"], s["obs_point"], s["meas"]) if obs is None else obs
    kw = dict(prior_pose=[0], prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None]) if prior0 else {}
    prob = StereoBAProblem(op.astype(np.int32), ol.astype(np.int32), meas, n, len(s["points_gt"]) if n_points is None else n_points,
                           s["K"], s["sigma"], pose_stride=3, band=band, between_span=span, loss=loss, **kw)
    return prob, NavBiasBASolver(prob, G.device(), window_prior=window)


# -- 1. the family stages ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage_scene(oracle):
    s = _scene(8, 400, 1)
    P, G = nbr.make_graph(oracle, s)
    rng = np.random.default_rng(7)
    poses, vels, biases = _displaced(oracle, rng, s)
    lam = 1e-3
    return s, P, G, (poses, vels, biases), lam, nbr.dense_system(oracle, s, P, G, poses, vels, biases, s["points_init"], lam)


def _padding_masks(nN, band):
    """Boolean masks of the entries of Sband [nN, band + 1, 6, 6] and gs [nN, 6] that belong to a velocity node's padding."""
    S, g = np.zeros((nN, band + 1, 6, 6), bool), np.zeros((nN, 6), bool)
    g[1::3, 3:] = True
    for q in range(nN):
        for sl in range(min(q, band) + 1):
            if q % 3 == 1:
                S[q, sl, 3:, :] = True
            if (q - sl) % 3 == 1:
                S[q, sl, :, 3:] = True
    return S.reshape(nN, band + 1, 36), g


@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("wide", [False, True])
def test_stages_against_the_reference(gpu, oracle, stage_scene, m, at_end, wide):
    s, P, G, (poses, vels, biases), lam, ref = stage_scene
    n = 8
    nN = 3 * n
    rng = np.random.default_rng(100 * m + 10 * at_end + wide)
    first, band = (n - m if at_end else 0), (20 if wide else max(3 * m - 1, 4))
    w = slice(first, first + m)
    W = fn.random_prior(rng, first, s["poses_gt"][w], s["vels_gt"][w], s["biases_gt"][w], singular=(m == 2))
    prob, sv = _solver(s, G, window=_device_prior(W, n), band=band)
    assert prob.band == band and prob.n_nodes == nN and len(sv._trial) == 5 + 4 * 2
    dl = fn.delta(oracle, W, poses, vels, biases).reshape(m, 15)
    assert np.abs(dl[:, :6]).max() > 0.02 and np.abs(dl[:, 6:9]).max() > 0.01 and np.abs(dl[:, 9:]).max() > 1e-3
    dposes, dvels, dbiases, dpoints = d(poses), d(vels), d(biases), d(s["points_init"])
    Href, gref, eref = fn.system(oracle, W, poses, vels, biases, n)
    assert relerr(sv.nav_window_prior_error(dposes, dvels, dbiases), eref) < STAGE_TOL
    sv.linearize(dposes, dpoints)
    sv.nav_linearize(dposes, dvels, dbiases)
    sv.nav_window_prior_linearize(dposes, dvels, dbiases)
    assert relerr(sv.nwp_scal[0].item(), eref) < STAGE_TOL
    assert relerr(sv.nwp_grad.cpu().numpy(), gref[fn.rows(first, m)]) < STAGE_TOL
    # assemble on top of a Schur result, twice: bit-identical, the padding entries untouched
    sv.Sband.fill_(float("nan"))
    sv.gs.fill_(float("nan"))
    sv.schur(lam)
    S0, g0 = sv.Sband.clone(), sv.gs.clone()
    runs = []
    for _ in range(2):
        sv.Sband.copy_(S0)
        sv.gs.copy_(g0)
        sv.nav_window_prior_assemble()
        runs.append((sv.Sband.cpu().numpy().copy(), sv.gs.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    padS, padg = _padding_masks(nN, band)
    S0n, g0n = S0.cpu().numpy(), g0.cpu().numpy()
    assert np.array_equal(runs[0][0][padS].view(np.int64), S0n[padS].view(np.int64))
    assert np.array_equal(runs[0][1][padg].view(np.int64), g0n[padg].view(np.int64))
    assert relerr(runs[0][0], S0n + nbr.band_blocks(Href, nN, band)) < STAGE_TOL
    assert relerr(runs[0][1].reshape(-1), g0n.reshape(-1) + gref) < STAGE_TOL
    # ... and with the inertial assemble after it: the whole damped system of the dense reference plus the prior
    sv.nav_assemble(lam)
    assert relerr(sv.Sband.cpu().numpy(), nbr.band_blocks(ref["A"] + Href, nN, band)) < STAGE_TOL
    assert relerr(sv.gs.cpu().numpy().reshape(-1), ref["g"] + gref) < STAGE_TOL
    # a step with all 18 coordinates of every keyframe non-zero (the padding's too: the family must not read it)
    x = 0.02 * rng.normal(size=18 * n)
    npo, nv, nb = nbr.retract(oracle, poses, vels, biases, x)
    sv.dp.copy_(d(x.reshape(nN, 6)))
    sv.new_poses.copy_(d(npo))
    sv.new_vels.copy_(d(nv))
    sv.new_bias.copy_(d(nb))
    outs = []
    for _ in range(2):
        sv.nwp_scal.fill_(float("nan"))
        sv.nav_window_prior_eval_step(dposes, dvels, dbiases)
        outs.append(sv.nwp_scal.cpu().numpy().copy())
    assert np.array_equal(outs[0][1:3].view(np.int64), outs[1][1:3].view(np.int64))
    assert relerr(outs[0][1], fn.linear_error(oracle, W, poses, vels, biases, x)) < STAGE_TOL
    assert relerr(outs[0][2], fn.error(oracle, W, npo, nv, nb)) < STAGE_TOL


def test_without_the_family_nothing_is_added(gpu, oracle, stage_scene):
    s, P, G = stage_scene[:3]
    _, sv = _solver(s, G)
    assert len(sv._trial) == 5 + 4 and "nav_window_prior" not in sv._families and not hasattr(sv, "nwp_grad")
    assert sv.nav_window_prior_error(None, None, None) == 0.0


# -- 2. vus_ba_band_marginalize on stride-3-shaped systems, and the compaction ------------------------------------------
@pytest.mark.parametrize("n,band,k", [(24, 20, 3), (30, 20, 9), (60, 26, 33)])
def test_band_marginalize_on_systems_with_identity_padding(gpu, n, band, k):
    """One partial panel, one panel boundary crossed, several panels (panels are 8 nodes).  Velocity nodes 3 i + 1 carry an
    identity on their last three coordinates and a zero gradient there."""
    rng = np.random.default_rng(1000 * band + 10 * k + n)
    A, _ = mr.random_spd_band(rng, n, band)
    b = rng.normal(size=6 * n) * np.abs(A).max()
    pad = fn.pad_rows(0, n // 3)
    A[pad], A[:, pad], b[pad] = 0.0, 0.0, 0.0
    A[pad, pad] = 1.0
    Href, gref, cref = fl.marginal_head(A, b, 0.0, k)
    H2, g2, c2 = fl.marginal_head(A, b, 0.0, k, one_at_a_time=True, solve="lu")
    tol = solve_tol(max(relerr(H2, Href), relerr(g2, gref), abs(c2 - cref) / abs(cref)))
    w = n - k
    f64 = dict(dtype=torch.float64, device="cuda")
    H, g, quad = torch.full((6 * w, 6 * w), float("nan"), **f64), torch.full((6 * w,), float("nan"), **f64), torch.full((1,), float("nan"), **f64)
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().vus_ba_band_marginalize_work_doubles(n, band, k)), **f64)
    assert work.numel() > 0
    p, st = _lib.ptr, _lib.current_stream_ptr()
    _lib.call("vus_ba_band_marginalize", p(d(mr.dense_to_band(A, band))), n, band, p(d(b.reshape(n, 6))), k, p(H), p(g), p(quad),
              p(status), p(work), st)
    assert int(status.item()) == 0
    Hn, gn = H.cpu().numpy(), g.cpu().numpy()
    print(f"n={n} band={band} n_drop={k}: H {relerr(Hn, Href):.2e} g {relerr(gn, gref):.2e} tol {tol:.2e}")
    assert relerr(Hn, Href) < tol and relerr(gn, gref) < tol and abs(-0.5 * float(quad.item()) - cref) < tol * abs(cref)
    # the padding rows of what is left come back as exact identity rows with a zero gradient
    kept_pad = pad[pad >= 6 * k] - 6 * k
    assert len(kept_pad) >= 3
    eye = np.eye(6 * w)
    assert np.array_equal(Hn[kept_pad], eye[kept_pad]) and np.array_equal(Hn[:, kept_pad], eye[:, kept_pad]) and not gn[kept_pad].any()
    if k % 3 == 0:          # whole keyframes dropped: the compaction of the rest against the statement's
        wk = w // 3
        H15, g15 = torch.full((15 * wk, 15 * wk), float("nan"), **f64), torch.full((15 * wk,), float("nan"), **f64)
        _lib.call("vus_nav_window_prior_compact", p(H), p(g), wk, p(H15), p(g15), st)
        Hc, gc, dev = fn.compact(Hn, gn)
        assert dev == 0.0 and np.array_equal(H15.cpu().numpy(), Hc) and np.array_equal(g15.cpu().numpy(), gc)


# -- 3. marginalisation is exact at the linearisation point -----------------------------------------------------------
N_KF = 10


@pytest.fixture(scope="module")
def scene(oracle):
    """10 keyframes, about 120 landmarks each seen from at most 4 consecutive keyframes, IMU + DVL + bias walk + the priors
    on keyframe 0 (pose, velocity, bias)."""
    s = _scene(N_KF, 600, 3, obs_per_kf=60)
    assert 80 <= len(s["points_gt"]) <= 160
    return s, nbr.make_graph(oracle, s)[1]


def _part(s, G, kf0, n, lm_ids, obs_mask, masks, prior0, loss, span, window=None):
    """The solver of a part of the scene: keyframes kf0 .. kf0 + n - 1, the landmarks lm_ids, the observations and inertial
    factors the masks select, the pose prior on keyframe 0 if asked; everything re-indexed."""
    lm_map = -np.ones(len(s["points_gt"]), np.int64)
    lm_map[lm_ids] = np.arange(len(lm_ids))
    op, ol = s["obs_pose"][obs_mask] - kf0, lm_map[s["obs_point"][obs_mask]]
    assert (op >= 0).all() and (op < n).all() and (ol >= 0).all()
    Gs = fn.sub_graph(G, kf0, n, **masks)
    prob, sv = _solver(s, Gs, window=window, span=span, loss=loss, prior0=prior0, n=n, obs=(op, ol, s["meas"][obs_mask]),
                       n_points=len(lm_ids))
    return prob, sv, Gs


def _undamped_step(sv, state):
    sv._linearize_all(state)
    sv._assemble_zero()
    sv.band_solve()
    sv.backsub()
    assert int(sv.status.item()) == 0
    return sv.dp.cpu().numpy().copy().reshape(-1), sv.dl.cpu().numpy().copy()


def _dense(oracle, sv, Gs, poses, vels, biases, extra=None):
    """Dense (A, b, e0) over [nodes, landmarks] of a solver's graph at its last linearisation: the stereo products the GPU
    left (robust weights included), the inertial factors and an optional node-side system by their numpy statements."""
    lin = {k: getattr(sv, k).cpu().numpy() for k in ("W", "V", "gl", "Hpp", "gp")}
    pk = sv.P.pk
    return fn.full_dense(oracle, lin, float(sv.scal[0].item()), pk["obs_pose"].cpu().numpy(), pk["obs_point"].cpu().numpy(), Gs,
                         poses, vels, biases, sv.P.n_points, extra)


def _masks(G, which):
    return dict(imu=which(G.imu_i), dvl=which(G.dvl_pose), vp=which(G.vp_idx), bb=which(G.bb_i), bp=which(G.bp_idx))


@pytest.mark.parametrize("loss", [None, ("huber", 1.0)], ids=["gaussian", "huber"])
@pytest.mark.parametrize("k", [1, 3])
def test_marginalisation_is_exact_at_the_linearisation_point(gpu, oracle, scene, loss, k):
    s, G = scene
    n, nL = N_KF, len(s["points_gt"])
    op, ol = s["obs_pose"], s["obs_point"]
    rng = np.random.default_rng(21)
    poses, vels, biases = s["poses_init"], s["vels_gt"] + 0.05 * rng.normal(size=(n, 3)), 0.005 * rng.normal(size=(n, 6))
    points = s["points_init"]
    every = lambda idx: np.ones(len(idx), bool)
    # the full graph
    _, full, _ = _part(s, G, 0, n, np.arange(nL), np.ones(len(op), bool), _masks(G, every), True, loss, 0)
    state = (d(poses), d(vels), d(biases), d(points))
    dp_full, dl_full = _undamped_step(full, state)
    A, b, e0 = _dense(oracle, full, G, poses, vels, biases)
    mf = full.marginals(*state, points_cov=False)
    cov_full = [x.cpu().numpy() for x in (mf.pose_cov, mf.vel_cov, mf.biases_cov)]
    # the absorbed set: every landmark an expired keyframe sees with all its observations, the pose prior, every inertial
    # factor that touches an expired keyframe (an ImuFactor or bias between-factor i reaches keyframe i + 1)
    gone = np.zeros(nL, bool)
    gone[ol[op < k]] = True
    obs_A = gone[ol]
    absorbed = lambda idx: idx < k
    nA = int(max(op[obs_A].max(), k)) + 1
    assert k < nA < n
    lm_A, lm_R = np.nonzero(gone)[0], np.nonzero(~gone)[0]
    assert len(lm_A) and len(lm_R)
    _, svA, GA = _part(s, G, 0, nA, lm_A, obs_A, _masks(G, absorbed), True, loss, nA)
    W = svA.marginalize_head(d(poses[:nA]), d(vels[:nA]), d(biases[:nA]), d(points[lm_A]), k)
    assert (W.first, W.m, W.n_poses, W.span) == (0, nA - k, nA - k, nA - k - 1)
    assert torch.equal(W.x0, d(poses[k:nA])) and torch.equal(W.v0, d(vels[k:nA])) and torch.equal(W.b0, d(biases[k:nA]))
    # the same by the dense statement, and the floor between its two orders of summation
    AA, bA, eA = _dense(oracle, svA, GA, poses[:nA], vels[:nA], biases[:nA])
    lmsA = list(range(18 * nA, len(bA)))
    H18, g18, cref = fl.marginal(AA, bA, eA, list(range(18 * k)) + lmsA)
    Href, gref, dev = fn.compact(H18, g18)
    H2, g2, c2, dev2 = fn.marginal_head(*fl.marginal(AA, bA, eA, lmsA, "lu"), k, one_at_a_time=True, solve="lu")
    assert dev == 0.0 and dev2 < 1e-15
    tolA = solve_tol(max(relerr(H2, Href), relerr(g2, gref), abs(c2 - cref) / abs(cref)))
    got = (W.H.cpu().numpy(), W.g.cpu().numpy(), W.c_const)
    print(f"k={k} loss={loss}: prior H {relerr(got[0], Href):.2e} g {relerr(got[1], gref):.2e} c {abs(got[2] - cref) / abs(cref):.2e} tol {tolA:.2e}")
    assert relerr(got[0], Href) < tolA and relerr(got[1], gref) < tolA and abs(got[2] - cref) < tolA * abs(cref)
    # the reduced graph: the rest + the prior
    from visual_underwater_slam_amd.ba import NavWindowPrior
    nR = n - k
    Wr = NavWindowPrior(0, W.x0, W.v0, W.b0, W.H, W.g, W.c_const, nR)
    kept = lambda idx: idx >= k
    _, red, GR = _part(s, G, k, nR, lm_R, ~obs_A, _masks(G, kept), False, loss, nR, window=Wr)
    state_R = (d(poses[k:]), d(vels[k:]), d(biases[k:]), d(points[lm_R]))
    dp_red, dl_red = _undamped_step(red, state_R)
    # floor: the full dense system solved directly against marginalised first, both on the CPU
    elim = list(range(18 * k)) + [18 * n + 3 * int(j) + c for j in lm_A for c in range(3)]
    keep = np.setdiff1d(np.arange(len(b)), elim)
    x_full = np.linalg.solve(A, -b)
    Hm, gm, _ = fl.marginal(A, b, e0, elim)
    x_red = np.linalg.solve(Hm, -gm)
    tol = solve_tol(relerr(x_red, x_full[keep]))
    step_full, step_red = dp_full[18 * k:].reshape(nR, 3, 6), dp_red.reshape(nR, 3, 6)
    errs = [relerr(step_red[:, q], step_full[:, q]) for q in range(3)] + [relerr(dl_red, dl_full[lm_R])]
    print(f"  step: poses {errs[0]:.2e} velocities {errs[1]:.2e} biases {errs[2]:.2e} landmarks {errs[3]:.2e} tol {tol:.2e}")
    assert max(errs) < tol
    assert relerr(dp_full, x_full[:18 * n]) < tol                            # and the GPU's full step is the dense one
    mr_ = red.marginals(*state_R, points_cov=False)
    cov_red = [x.cpu().numpy() for x in (mr_.pose_cov, mr_.vel_cov, mr_.biases_cov)]
    cov_ref = np.linalg.inv(Hm)[:18 * nR, :18 * nR]
    tol_cov = solve_tol(relerr(np.linalg.inv(A)[np.ix_(keep, keep)][:18 * nR, :18 * nR], cov_ref))
    cerr = [relerr(cr, cf[k:]) for cr, cf in zip(cov_red, cov_full)]
    print(f"  pose_cov {cerr[0]:.2e} vel_cov {cerr[1]:.2e} biases_cov {cerr[2]:.2e} tol {tol_cov:.2e}")
    assert max(cerr) < tol_cov
    # prior on prior: the kept state displaced (delta != 0), the head of the reduced graph marginalised again -- against the
    # numpy statement doing the same two steps from its own first prior
    r3 = np.random.default_rng(3)
    mp = np.stack([oracle.pose_retract(T, 0.01 * r3.standard_normal(6)) for T in poses[k:]])
    mv, mb = vels[k:] + 0.01 * r3.standard_normal((nR, 3)), biases[k:] + 1e-3 * r3.standard_normal((nR, 6))
    W2 = red.marginalize_head(d(mp), d(mv), d(mb), d(points[lm_R]), 1)
    prior1 = fn.NavPrior(0, poses[k:nA].copy(), vels[k:nA].copy(), biases[k:nA].copy(), Href, gref, cref)
    dl1 = fn.delta(oracle, prior1, mp, mv, mb).reshape(-1, 15)
    assert min(np.abs(dl1[:, :6]).max(), np.abs(dl1[:, 6:9]).max(), np.abs(dl1[:, 9:]).max()) > 1e-4
    AR, bR, eR = _dense(oracle, red, GR, mp, mv, mb, extra=fn.system(oracle, prior1, mp, mv, mb, nR))
    lmsR = list(range(18 * nR, len(bR)))
    H18, g18, c3 = fl.marginal(AR, bR, eR, list(range(18)) + lmsR)
    H3, g3, _ = fn.compact(H18, g18)
    H4, g4, c4, _ = fn.marginal_head(*fl.marginal(AR, bR, eR, lmsR, "lu"), 1, one_at_a_time=True, solve="lu")
    tol2 = solve_tol(max(relerr(H4, H3), relerr(g4, g3), abs(c4 - c3) / abs(c3), tolA / 100.0))
    got = (W2.H.cpu().numpy(), W2.g.cpu().numpy(), W2.c_const)
    print(f"  prior on prior: H {relerr(got[0], H3):.2e} g {relerr(got[1], g3):.2e} c {abs(got[2] - c3) / abs(c3):.2e} tol {tol2:.2e}")
    assert W2.m == nR - 1
    assert relerr(got[0], H3) < tol2 and relerr(got[1], g3) < tol2 and abs(got[2] - c3) < tol2 * abs(c3)
    # the LM loop carries the family as one more term: its record has the slot, the error of the state it returns is the sum
    # of the three statements, and the step it accepts lowers it
    out = red.optimize(*state_R)
    rep = out[-1]
    fp, fv, fb = (x.cpu().numpy() for x in out[:3])
    assert len(red._trial) == 5 + 4 * 2 and rep.iterations >= 1 and rep.final_error < rep.initial_error
    held = prior1._replace(H=W.H.cpu().numpy(), g=W.g.cpu().numpy(), c=W.c_const)          # the prior the reduced graph holds
    parts = red.error(out[0], out[3]) + red.nav_error(*out[:3]) + fn.error(oracle, held, fp, fv, fb)
    assert abs(parts - rep.final_error) < 1e-9 * rep.final_error


# -- 5. refusals on the device path ----------------------------------------------------------------------------------------
def test_the_check_refuses_a_bad_prior_by_name(gpu, oracle, stage_scene):
    s, P, G = stage_scene[:3]
    n, m = 8, 2
    rng = np.random.default_rng(6)
    W = fn.random_prior(rng, 1, s["poses_gt"][1:3], s["vels_gt"][1:3], s["biases_gt"][1:3])

    def build(**kw):
        return _solver(s, G, window=_device_prior(W._replace(**kw), n), span=m)
    build()
    Z = W.H.copy()
    Z[7], Z[:, 7] = 0.0, 0.0                          # positive semi-definite with a free direction: accepted
    build(H=Z)
    A = W.H.copy()
    A[2, 20] += 1e-6 * np.abs(W.H).max()
    bad = W.H.copy()
    bad[3, 3] = float("nan")
    neg = W.H.copy()
    neg[8, 8] = -1e-3
    v0 = W.v0.copy()
    v0[1, 2] = np.inf
    b0 = W.b0.copy()
    b0[0, 0] = np.nan
    for kw, word in ((dict(H=A), "not symmetric"), (dict(H=bad), "not finite"), (dict(H=neg), "negative diagonal"),
                     (dict(g=np.r_[np.inf, np.zeros(15 * m - 1)]), "not finite"), (dict(c=float("inf")), "not finite"),
                     (dict(v0=v0), "v0 of keyframe 1"), (dict(b0=b0), "b0 of keyframe 0")):
        with pytest.raises(_lib.VusError, match=word):
            build(**kw)
    with pytest.raises(ValueError, match="between_span=2"):          # the scene's own band of 4 nodes: 3 m - 1 = 5 does not fit
        _solver(s, G, window=_device_prior(W, n))


def test_marginalize_head_refuses_what_it_cannot_serve(gpu, oracle, stage_scene):
    from visual_underwater_slam_amd.ba import IndeterminantSystem
    s, P, G = stage_scene[:3]
    n = 8
    state = (d(s["poses_init"]), d(s["vels_gt"]), d(np.zeros((n, 6))), d(s["points_init"]))
    _, narrow = _solver(s, G)
    with pytest.raises(ValueError, match="between_span=7"):
        narrow.marginalize_head(*state, 1)
    _, sv = _solver(s, G, span=n)
    for k in (0, n):
        with pytest.raises(ValueError, match="n_drop"):
            sv.marginalize_head(*state, k)
    # no bias between-factors: B(1) has neither a prior nor a between-factor
    Gf = nbr.make_graph(oracle, s, with_between=False)[1]
    _, free = _solver(s, Gf, span=n)
    with pytest.raises(IndeterminantSystem) as e:
        free.marginalize_head(*state, 2)
    assert (e.value.kind, e.value.index) == ("bias", 1)
    W = free.marginalize_head(*state, 1)              # B(0) has its prior: dropping it alone is served
    assert W.m == n - 1
    # marginals(): a NavWindowPrior over every keyframe counts their biases as constrained
    with pytest.raises(IndeterminantSystem) as e:
        free.marginals(*state, points_cov=False)
    assert (e.value.kind, e.value.index) == ("bias", 1)
    rng = np.random.default_rng(8)
    Wall = fn.random_prior(rng, 0, s["poses_gt"], s["vels_gt"], s["biases_gt"])
    _, held = _solver(s, Gf, window=_device_prior(Wall, n), span=n)
    assert held.marginals(*state, points_cov=False).biases_cov.shape == (n, 6, 6)


# -- 4. the smoother end to end -----------------------------------------------------------------------------------------
def _keyframe_factors(s, i, pims):
    """The factors keyframe i brings: the priors on keyframe 0, else ImuFactor(i - 1 -> i, B(i - 1)), the bias walk
    B(i - 1) -> B(i) and the DVL on (V(i), X(i)); and its stereo factors."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B, L
    nm, cfg = gtsam.noiseModel, fn.SMOOTHER
    out = []
    if i == 0:
        out += [gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(s["poses_gt"][0]), nm.Diagonal.Sigmas(s["prior_sigmas"])),
                gtsam.PriorFactorVector(V(0), s["vels_gt"][0], nm.Isotropic.Sigma(3, cfg["vprior_sigma"])),
                gtsam.PriorFactorConstantBias(B(0), gtsam.imuBias.ConstantBias(),
                                              nm.Diagonal.Sigmas(np.repeat(cfg["bias_prior_sigma"], 3)))]
    else:
        out += [gtsam.ImuFactor(X(i - 1), V(i - 1), X(i), V(i), B(i - 1), pims[i - 1]),
                gtsam.BetweenFactorConstantBias(B(i - 1), B(i), gtsam.imuBias.ConstantBias(), nm.Diagonal.Sigmas(np.repeat(fn.WALK, 3))),
                gtsam.DvlVelocityFactor(nm.Isotropic.Sigma(3, cfg["dvl_sigma"]), V(i), X(i), s["dvl"][i])]
    K, noise = gtsam.Cal3_S2Stereo(*s["K"]), nm.Isotropic.Sigma(3, cfg["stereo_sigma"])
    rows = np.nonzero(s["obs_pose"] == i)[0]
    return out + [gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*s["meas"][a]), noise, X(i), L(int(s["obs_point"][a])), K)
                  for a in rows], rows


def _pims(s):
    from visual_underwater_slam_amd import gtsam
    params = gtsam.PreintegrationParams.MakeSharedU(9.81)
    params.setAccelerometerCovariance(nbr.ACC_COV); params.setGyroscopeCovariance(nbr.GYRO_COV)
    params.setIntegrationCovariance(nbr.INT_COV)
    out = []
    for samples in s["imu"]:
        pim = gtsam.PreintegratedImuMeasurements(params, gtsam.imuBias.ConstantBias())
        for smp in samples:
            pim.integrateMeasurement(smp[:3], smp[3:6], smp[6])
        out.append(pim)
    return out


def test_the_inertial_smoother_follows_the_full_batch(gpu):
    """16 keyframes with IMU, DVL, a bias walk and stereo factors, lag = 6 keyframes, one keyframe per update, noise drawn at
    the stated sigmas (fixed_lag_nav_ref.smoother_scene).  The newest position of the smoother lies within ONE standard
    deviation of its batch marginal of the full-batch optimum -- test_fixed_lag_gpu.py's criterion."""
    from visual_underwater_slam_amd import gtsam, gtsam_unstable
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B, L
    s = fn.smoother_scene()
    n, lag = fn.SMOOTHER["n"], float(fn.SMOOTHER["lag"])
    pims = _pims(s)
    # the full batch
    graph, init = gtsam.NonlinearFactorGraph(), gtsam.Values()
    for i in range(n):
        init.insert(X(i), gtsam.Pose3.from_flat12(s["poses_init"][i]))
        init.insert(V(i), s["vels_gt"][0].copy())
        init.insert(B(i), gtsam.imuBias.ConstantBias())
        for f in _keyframe_factors(s, i, pims)[0]:
            graph.push_back(f)
    for j in range(len(s["points_gt"])):
        init.insert(L(j), s["points_init"][j])
    batch = gtsam.LevenbergMarquardtOptimizer(graph, init, gtsam.LevenbergMarquardtParams()).optimize()
    cov = gtsam.Marginals(graph, batch).marginalCovariance(X(n - 1))
    one_sigma = float(np.sqrt(np.trace(cov[3:, 3:])))
    want = batch.atPose3(X(n - 1)).translation()

    sm = gtsam_unstable.BatchFixedLagSmoother(lag)
    present, live, ts, first_seen = set(), set(), {}, {}
    cases = dict(marginalised=0, discarded=0)
    for i in range(n):
        factors, rows = _keyframe_factors(s, i, pims)
        g, theta = gtsam.NonlinearFactorGraph(), gtsam.Values()
        for f in factors:
            g.push_back(f)
        theta.insert(X(i), gtsam.Pose3.from_flat12(s["poses_init"][i]))
        theta.insert(V(i), sm.calculateEstimate().atVector(V(i - 1)) if i else s["vels_gt"][0].copy())
        theta.insert(B(i), sm.calculateEstimate().atConstantBias(B(i - 1)) if i else gtsam.imuBias.ConstantBias())
        stamps = {k: float(i) for k in (X(i), V(i), B(i))}
        ts[("x", i)] = float(i)
        for a in rows:
            j = int(s["obs_point"][a])
            if j not in present:
                present.add(j)
                first_seen[j] = i
                theta.insert(L(j), s["points_init"][j])
            new_stamp = fn.landmark_stamp(j, first_seen[j], i)
            if ts.get(j) != new_stamp:
                ts[j] = stamps[L(j)] = new_stamp
            live.add((i, j))
        stats = sm.update(g, theta, stamps)
        cut = float(i) - lag
        expired = {p for p in range(i + 1) if ("x", p) in ts and ts[("x", p)] < cut}
        seen = {j for p, j in live if p in expired}
        gone = {j for j in seen if ts[j] < cut}
        discarded = {(p, j) for p, j in live if p in expired and j not in gone}
        cases["marginalised"] += len(gone)
        cases["discarded"] += len(discarded)
        assert (stats["expired_poses"], stats["marginalized_landmarks"], stats["discarded_factors"]) == \
            (len(expired), len(gone), len(discarded)), i
        live = {(p, j) for p, j in live if p not in expired and j not in gone}
        present -= gone
        for p in expired:
            del ts[("x", p)]
        est = sm.calculateEstimate()
        window = [int(k) for k in est._pose3_table()[0]]
        assert len(window) == min(i + 1, int(lag) + 1) and window[-1] == X(i)
        for k in window:                             # every keyframe of the window holds all three keys, with one timestamp
            kx, kv, kb = gtsam_unstable.keyframe_keys(k)
            assert est.exists(kv) and est.exists(kb) and sm.timestamps()[kv] == sm.timestamps()[kb] == sm.timestamps()[kx]
        assert all(not est.exists(k) for p in expired for k in (X(p), V(p), B(p))) and all(not est.exists(L(j)) for j in gone)
        containers = [f for f in sm.getFactors()._factors if isinstance(f, gtsam.LinearContainerFactor)]
        assert len(containers) == int(i > lag)
        if containers:                               # over X, V, B of leading keyframes of the window
            ck = sorted(containers[0].keys())
            m = len(ck) // 3
            assert containers[0]._is_inertial() and ck == sorted(k for p in window[:m] for k in gtsam_unstable.keyframe_keys(p))
    assert min(cases.values()) > 0, cases
    diff = float(np.linalg.norm(sm.calculateEstimatePose3(X(n - 1)).translation() - want))
    sec = sm.last_update["seconds"]
    print(f"newest position against the batch: smoother {diff:.4e} m = {diff / one_sigma:.3f} sigma (one sigma = {one_sigma:.4e} m); "
          f"cases {cases}; last update pack {sec['pack']:.3f} s optimise {sec['optimize']:.3f} s marginalise {sec['marginalize']:.3f} s")
    assert diff <= one_sigma


def test_a_dropped_bias_without_information_is_named_by_its_key(gpu):
    """No bias factor at all: when keyframe 0 expires, B(0) has neither a prior nor a between-factor, and the smoother names it."""
    from visual_underwater_slam_amd import gtsam, gtsam_unstable
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B, L
    s = fn.smoother_scene()
    pims = _pims(s)
    sm = gtsam_unstable.BatchFixedLagSmoother(1.0)
    seen = set()
    for i in range(3):
        factors, rows = _keyframe_factors(s, i, pims)
        g, theta = gtsam.NonlinearFactorGraph(), gtsam.Values()
        for f in factors:
            if not isinstance(f, (gtsam.PriorFactorConstantBias, gtsam.BetweenFactorConstantBias)):
                g.push_back(f)
        theta.insert(X(i), gtsam.Pose3.from_flat12(s["poses_init"][i]))
        theta.insert(V(i), s["vels_gt"][i].copy())
        theta.insert(B(i), gtsam.imuBias.ConstantBias())
        stamps = {k: float(i) for k in (X(i), V(i), B(i))}
        for a in rows:
            j = int(s["obs_point"][a])
            if j not in seen:
                seen.add(j)
                theta.insert(L(j), s["points_init"][j])
                stamps[L(j)] = float(i)
        if i < 2:
            sm.update(g, theta, stamps)
            continue
        with pytest.raises(gtsam.IndeterminantLinearSystemException) as e:
            sm.update(g, theta, stamps)
        assert e.value.key == B(0)
