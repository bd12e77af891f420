"""Long loop closures as a low-rank correction of the band solve (include/vus_closure.h, ba.BetweenFactors(max_span=...),
the solver hook, the gtsam shim, run_sequence) on the MI355X.

vus_ba_band_resolve: further right-hand sides against the factor the one-sided band solve leaves in Sband, held against
numpy.linalg.solve with the dense system.  On every system the existing vus_ba_band_solve_multi solves the first <= 8 of the
same columns; its relative error against the same dense solve is the yardstick: the new call may be at most 8 x that error,
never tighter than 1e-13 (both do the same operations, the order of the sums differs).

The stage kernels against tests/closure_ref.py; one trial at a fixed lambda against the dense solve of between_ref.system
AND against the existing widened-band solver on the same graph (the new path's error may be at most 8 x the widened path's,
floor 1e-12); the LM loop against the decision logs test_closure_ref.py certifies on the CPU; band, storage and band mode;
the defaults; the shim and run_sequence; the refusals.  Every measured figure is printed before its assertion
(profiles/long_closures.md holds them)."""
import functools

import numpy as np
import pytest
import torch

import closure_ref as cr
import marginals_ref as mr

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def system(n, band):
    """(dense A, band storage, 384 right-hand sides, their dense solutions): computed once per shape, never modified."""
    rng = np.random.default_rng(7000 + 1000 * n + band)
    A, Sb = mr.random_spd_band(rng, n, band)
    B = rng.normal(size=(cr.RESOLVE_COLS[-1], 6 * n))
    ref = np.linalg.solve(A, B.T).T
    for a in (A, Sb, B, ref):
        a.setflags(write=False)
    return A, Sb, B, ref


def factor(Sb, band, rhs):
    """One-sided band solve of `rhs` (<= 8 rows, solved in place): the factor it leaves, as a device tensor."""
    from visual_underwater_slam_amd import _lib
    n = Sb.shape[0]
    d_S = torch.tensor(Sb, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.call("vus_ba_band_solve_multi", d_S.data_ptr(), n, band, rhs.data_ptr(), rhs.shape[0], st.data_ptr(),
              _lib.current_stream_ptr())
    assert int(st.item()) == 0
    return d_S


def resolve(d_L, n, band, X, n_cols):
    from visual_underwater_slam_amd import _lib
    _lib.call("vus_ba_band_resolve", d_L.data_ptr(), n, band, X.data_ptr(), n_cols, None, 0, _lib.current_stream_ptr())


@pytest.mark.parametrize("n_cols", cr.RESOLVE_COLS)
@pytest.mark.parametrize("n,band", cr.RESOLVE_SHAPES)
def test_resolve_against_the_dense_solve(gpu, n, band, n_cols):
    A, Sb, B, ref = system(n, band)
    k = min(8, n_cols)
    rhs = torch.from_numpy(B[:k].copy()).cuda()
    d_L = factor(Sb, band, rhs)
    base = relerr(rhs.cpu().numpy(), ref[:k])
    L_before = d_L.clone()
    # two sentinel rows behind the n_cols the call owns
    X = torch.full((n_cols + 2, 6 * n), 12345.0, dtype=torch.float64, device="cuda")
    X[:n_cols] = torch.from_numpy(B[:n_cols].copy()).cuda()
    X2 = X.clone()
    resolve(d_L, n, band, X, n_cols)
    resolve(d_L, n, band, X2, n_cols)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    err = relerr(got[:n_cols], ref[:n_cols])
    print(f"resolve n={n} band={band} n_cols={n_cols}: band_solve_multi {base:.3e}  band_resolve {err:.3e}")
    assert err <= max(8.0 * base, 1e-13)
    assert torch.equal(d_L.view(torch.int64), L_before.view(torch.int64)), "the factor was modified"
    assert torch.equal(X.view(torch.int64), X2.view(torch.int64)), "two calls differ"
    assert (got[n_cols:] == 12345.0).all(), "rows beyond n_cols were written"


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("n,band", [(130, 30), (300, 224)])
def test_every_band_mode_leaves_the_layout_resolve_reads(gpu, band_tuning, n, band, mode):
    band_tuning(band_mode=mode)
    A, Sb, B, ref = system(n, band)
    rhs = torch.from_numpy(B[:8].copy()).cuda()
    d_L = factor(Sb, band, rhs)
    base = relerr(rhs.cpu().numpy(), ref[:8])
    X = torch.from_numpy(B[:17].copy()).cuda()
    resolve(d_L, n, band, X, 17)
    err = relerr(X.cpu().numpy(), ref[:17])
    print(f"resolve n={n} band={band} band mode {mode}: band_solve_multi {base:.3e}  band_resolve {err:.3e}")
    assert err <= max(8.0 * base, 1e-13)


# ---- the long set -------------------------------------------------------------------------------------------------------
import between_ref as br
import lm_ref


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def no_points():
    return torch.zeros((0, 3), dtype=torch.float64, device="cuda")


def measured(rng, truth, pairs, noise, losses=None, sig=(0.01, 0.01, 0.01, 0.05, 0.05, 0.05)):
    """A between_ref.BetweenSet measured from `truth` with tangent noise."""
    from visual_underwater_slam_amd.gtsam import Pose3
    meas = [Pose3.from_flat12(truth[a]).between(Pose3.from_flat12(truth[b])).retract(noise * rng.standard_normal(6)).flat12()
            for a, b in pairs]
    return br.BetweenSet([a for a, _ in pairs], [b for _, b in pairs], np.array(meas), np.tile(sig, (len(pairs), 1)), losses)


def device_set(G, n, stride=1, max_span=None):
    from visual_underwater_slam_amd.ba import BetweenFactors
    return BetweenFactors(G.i, G.j, G.meas, 1.0 / G.w, n, pose_stride=stride, loss=list(G.losses), max_span=max_span)


def pose_only(G, priors, n, max_span=None):
    """(problem, solver) of a pose graph: no landmarks, the band is the between factors' (the in-band ones' with max_span)"""
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    bf = device_set(G, n, max_span=max_span)
    z = np.zeros((0,))
    prob = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                           prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=bf.span)
    return prob, StereoBASolver(prob, bf)


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_stage_kernels_against_the_reference(gpu, oracle, stride):
    """Both key orders, two long factors on one pair, two sharing a node, one exactly one pose outside the band; Cauchy,
    Huber and Gaussian factors in one set.  rows / err at the 1e-12 test_between_gpu.py asks of `lin`; gs and U are exact
    placements; C and the corrected columns against numpy on the GPU's own rows at 1e-11 of the largest entry.  The band
    system is a random SPD band scaled to the size of U U^T, so that the dense reference's own error (cond x eps) stays
    under that bound."""
    from visual_underwater_slam_amd import _lib
    rng = np.random.default_rng(20 + stride)
    n, M = 30, 5
    truth, init, _, _ = br.pose_graph(rng, n)
    long_pairs = [(2, 20), (20, 2), (2, 20), (2, 27), (10, 16), (25, 8)]
    long_losses = [(2, 0.5), (0, 0.0), (1, 0.3), (2, 1.0), (0, 0.0), (1, 1.345)]
    pairs = [(k - 1, k) for k in range(1, n)] + [(3, 7)] + long_pairs
    G = measured(rng, truth, pairs, 0.02, [(0, 0.0)] * n + long_losses)
    bf = device_set(G, n, stride, max_span=M)
    Lg, (Gin, Glong) = bf.long, cr.split(G, M)
    assert bf.n == n and bf.span == 4 and Lg.n == 6 and Lg.min_span == M + 1
    nN, band, m = stride * n, stride * M, 36
    st, p = _lib.current_stream_ptr(), _lib.ptr
    _lib.call("vus_closure_check", Lg.addr(), band, st)
    with pytest.raises(_lib.VusError, match="inside the band"):
        _lib.call("vus_closure_check", Lg.addr(), stride * (M + 1), st)
    poses = d(init)
    f64 = dict(dtype=torch.float64, device="cuda")
    rows, sc = torch.empty((6, 78), **f64), torch.zeros(4, **f64)
    work = torch.empty(int(_lib.load().vus_closure_work_doubles(Lg.addr())), **f64)
    _lib.call("vus_closure_linearize", Lg.addr(), p(poses), p(rows), p(sc), p(work), st)
    H, g, e0, fac = br.system(oracle, Glong, init, nN, stride)
    R = rows.cpu().numpy()
    assert relerr(R, cr.rows(fac)) < 1e-12 and abs(sc[0].item() - e0) < 1e-12 * e0
    gs = torch.zeros((nN, 6), **f64)
    _lib.call("vus_closure_gradient", Lg.addr(), p(rows), p(gs), st)
    got = gs.cpu().numpy()
    assert relerr(got.reshape(-1), g) < 1e-12
    touched = np.zeros(nN, bool)
    touched[stride * np.r_[Glong.i, Glong.j]] = True
    assert (got[~touched] == 0.0).all()
    U = torch.full((m, 6 * nN), float("nan"), **f64)
    _lib.call("vus_closure_scatter", Lg.addr(), p(rows), p(U), st)
    want = np.zeros((m, 6 * nN))
    for f, (a, b) in enumerate(long_pairs):
        want[6 * f:6 * f + 6, 6 * stride * a:6 * stride * a + 6] = R[f, :36].reshape(6, 6)
        want[6 * f:6 * f + 6, 6 * stride * b:6 * stride * b + 6] = R[f, 36:72].reshape(6, 6)
    Un = U.cpu().numpy()
    assert np.array_equal(Un, want)
    # the band system B, its factor, Z = B^-1 U, C and the corrected columns
    A, Sb = mr.random_spd_band(rng, nN, band)
    scale = np.abs(Un.T @ Un).max() / np.abs(A).max()
    A, Sb = scale * A, scale * Sb
    b = rng.normal(size=(2, 6 * nN))
    X = d(b)
    d_L = factor(Sb, band, X)
    resolve(d_L, nN, band, U, m)
    C = torch.empty((m, m), **f64)
    _lib.call("vus_closure_capacitance", Lg.addr(), p(rows), p(U), p(C), st)
    Zref = np.linalg.solve(A, Un.T)
    Cref = np.eye(m) + Un @ Zref
    Cg = C.cpu().numpy()
    Lc = np.tril(Cg)
    e_fac = np.abs(Lc @ Lc.T - Cref).max() / np.abs(Cref).max()
    e_up = np.abs(np.triu(Cg, 1) - np.triu(Cref, 1)).max() / np.abs(Cref).max()
    _lib.call("vus_closure_correct", Lg.addr(), p(rows), p(U), p(C), p(X), 2, p(work), st)
    xref = np.linalg.solve(A + Un.T @ Un, b.T).T
    e_x = relerr(X.cpu().numpy(), xref)
    print(f"stride {stride}: Z {relerr(U.cpu().numpy(), Zref.T):.2e}, C = L L^T {e_fac:.2e}, upper triangle {e_up:.2e}, corrected columns "
          f"{e_x:.2e}; cond(B + U U^T) {np.linalg.cond(A + Un.T @ Un):.2e}")
    assert e_fac <= 1e-11 and e_up <= 1e-11 and e_x <= 1e-11


# ---- one trial at a fixed lambda: the new path, the widened band, the dense solve -------------------------------------------
LAM = 1e-3


def trial(sv, state):
    sv._lm_linearize(state)
    sv._lm_solve(LAM)
    assert int(sv.status.item()) == 0
    return sv.dp.cpu().numpy().reshape(-1), sv.dl.cpu().numpy()


def held_to_the_widened_path(name, what, got_long, got_wide, ref):
    e_long, e_wide = relerr(got_long, ref), relerr(got_wide, ref)
    print(f"{name}: {what} against the dense solve: long closures as a low-rank term {e_long:.3e}, widened band {e_wide:.3e}")
    assert e_long <= max(8.0 * e_wide, 1e-12), (name, what, e_long, e_wide)


@pytest.mark.parametrize("name", ["closure-40", "closures-400"])
def test_one_trial_of_a_pose_graph(gpu, oracle, name):
    truth, init, G, priors = cr.lm_case(name)
    n = len(init)
    A0, g0, _ = br.prior_system(oracle, priors, init)
    H, g, _, _ = br.system(oracle, G, init, n)
    ref = np.linalg.solve(A0 + LAM * np.eye(6 * n) + H, -(g0 + g))
    state = (d(init), no_points())
    prob_l, sv_l = pose_only(G, priors, n, max_span=cr.LM_MAX_SPAN)
    prob_w, sv_w = pose_only(G, priors, n)
    assert prob_l.band == 1 and prob_w.band == G.span and sv_l.C.n == len(cr.LM_CASES[name]["closures"])
    held_to_the_widened_path(name, "dp", trial(sv_l, state)[0], trial(sv_w, state)[0], ref)


@functools.lru_cache(maxsize=None)
def stereo_200():
    """200 keyframes, 3000 landmarks (the stereo + between graph of test_between_gpu.py), its landmark band, and 64 closures
    wider than that band, both key orders, spread over the trajectory"""
    import nav_ref
    from visual_underwater_slam_amd import synth
    seq = synth.ba_sequence(200, 3000, 300)
    span = nav_ref.pose_band(seq["obs_pose"], seq["obs_point"])
    far = [(k, k + span + 1 + k % 21) if k % 2 else (k + span + 1 + k % 21, k) for k in range(64)]
    assert all(abs(a - b) > span and max(a, b) < 200 for a, b in far)
    return seq, span, far


@functools.lru_cache(maxsize=None)
def stereo_dense_200(oracle):
    from visual_underwater_slam_amd import ba_pack
    seq, span, _ = stereo_200()
    n, nL = 200, len(seq["points_gt"])
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]),
                                   torch.from_numpy(seq["meas"]), n, nL)
    P = oracle.BAProblem(pk, seq["K"], seq["sigma"], (np.array([0], np.int32), seq["poses_init"][:1], seq["prior_sigmas"][None]))
    A, g, lin, sch = br.stereo_dense(oracle, P, seq["poses_init"], seq["points_init"], span, LAM)
    return P, A, g, lin, sch


@pytest.mark.parametrize("k", [1, 3, 64])
def test_one_trial_of_stereo_plus_between(gpu, oracle, k):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    seq, span, far = stereo_200()
    n, nL = 200, len(seq["points_gt"])
    P, A, g, lin, sch = stereo_dense_200(oracle)
    rng = np.random.default_rng(30 + k)
    G = measured(rng, seq["poses_gt"], [(i - 1, i) for i in range(1, n)] + far[:k], 0.01)
    H, gb, _, _ = br.system(oracle, G, seq["poses_init"], n)
    x = np.linalg.solve(A + H, -(g + gb))
    dl_ref = oracle.ba_backsub(P, lin, sch["Vinv"], x.reshape(n, 6))
    state = (d(seq["poses_init"]), d(seq["points_init"]))
    got = {}
    for which, max_span in (("long", span), ("wide", None)):
        bf = device_set(G, n, max_span=max_span)
        prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                               prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        assert prob.band == (span if max_span else G.span) and (sv.C.n == k if max_span else sv.C is None)
        got[which] = trial(sv, state)
    held_to_the_widened_path(f"stereo + {k} long closures", "dp", got["long"][0], got["wide"][0], x)
    held_to_the_widened_path(f"stereo + {k} long closures", "dl", got["long"][1], got["wide"][1], dl_ref)


@pytest.mark.parametrize("stride", [2, 3])
def test_one_trial_of_the_inertial_solvers(gpu, oracle, stride):
    """NavBASolver (the correction runs on all 7 columns before the bias border) and NavBiasBASolver, 24 keyframes whose
    landmark band is 21 poses, closures 23 and 22 poses long."""
    import nav_ref
    import nav_bias_ref as nbr
    from visual_underwater_slam_amd import synth
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavBiasBASolver, NavFactors
    s = synth.nav_sequence(24, 300, 60)
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    span = nav_ref.pose_band(s["obs_pose"], s["obs_point"])
    rng = np.random.default_rng(40 + stride)
    G = measured(rng, s["poses_gt"], [(i - 1, i) for i in range(1, n)] + [(0, 23), (23, 1)], 0.01)
    assert span == 21
    vels = np.zeros((n, 3))
    if stride == 3:
        P, NG = nbr.make_graph(oracle, s)
        bias = np.zeros((n, 6))
        ref = nbr.dense_system(oracle, s, P, NG, s["poses_init"], vels, bias, s["points_init"], LAM, band=span)
        make = lambda prob, bf: NavBiasBASolver(prob, NG.device(), bf)
    else:
        from test_nav_oracle import build_nav
        P, _ = build_nav(oracle, s)
        pims, Ws = nbr.preintegrate(s)
        imu = (np.arange(n - 1), np.arange(1, n), pims, Ws)
        dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
        vpr = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
        bias = np.zeros(6)
        ref = nav_ref.dense_system(oracle, s, P, oracle.NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr), s["poses_init"], vels,
                                   bias, s["points_init"], LAM)
        make = lambda prob, bf: NavBASolver(prob, NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr), bf)
    nc = 6 * stride * n
    H, gb, _, _ = br.system(oracle, G, s["poses_init"], stride * n, stride)
    A, g = ref["A"].copy(), ref["g"].copy()
    A[:nc, :nc] += H
    g[:nc] += gb
    x = np.linalg.solve(A, -g)[:nc]
    state = (d(s["poses_init"]), d(vels), d(bias), d(s["points_init"]))
    got = {}
    for which, max_span in (("long", span), ("wide", None)):
        bf = device_set(G, n, stride, max_span=max_span)
        prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                               prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=stride,
                               between_span=bf.span)
        sv = make(prob, bf)
        assert (sv.C.n == 2 and prob.band == stride * span) if max_span else sv.C is None
        got[which] = trial(sv, state)[0]
    held_to_the_widened_path(f"inertial, pose_stride {stride}", "dp", got["long"], got["wide"], x)


# ---- the LM loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.LM_CASES))
def test_lm_decisions_equal_the_references_and_the_widened_band(gpu, oracle, monkeypatch, name):
    """The decision sequence and lambda history of both GPU paths are those of the dense CPU loop (between_ref.lm_optimize,
    as lm_ref.replay walks it) -- exactly: test_closure_ref.py certifies every decision 1e-3 away from its threshold.
    Values by the rule of test_lm_branches_gpu.py: 100 x the floor between the two CPU references (the dense solve and
    the low-rank one), never tighter than 1e-11 (kernels) / 1e-8 (after a solve)."""
    from test_lm_branches_gpu import Recorder
    from visual_underwater_slam_amd.ba import LMParams
    truth, init, G, priors = cr.lm_case(name)
    n, prm = len(init), cr.LM_CASES[name]["params"]
    dense, low = (lm_ref.replay(cr.PoseGraphStages(oracle, G, priors, init, max_span=m), **prm) for m in (None, cr.LM_MAX_SPAN))
    floor = lm_ref.value_differences(dense, low)
    tol = lm_ref.tolerance(floor)
    for which, max_span in (("long", cr.LM_MAX_SPAN), ("wide", None)):
        prob, sv = pose_only(G, priors, n, max_span=max_span)
        rec = Recorder(sv, monkeypatch.setattr)
        poses, _, rep = sv.optimize(d(init), no_points(), LMParams(**prm))
        log = rec.log((poses,), rep)
        assert [(t["lam"], t["outcome"], t["status"]) for t in log["trials"]] == lm_ref.outcomes(dense), which
        assert rep.lambda_hist == dense["lambda_hist"] and rep.status == dense["status"]
        assert rep.long_closures == (sv.C.n if max_span else 0)
        got = {"lin0": 0.0, "scalars": 0.0, "state": relerr(log["state"][0], dense["state"][0])}
        for a, b in zip(log["trials"], dense["trials"]):
            key = "scalars" if a["outer"] else "lin0"
            got[key] = max(got[key], lm_ref.relerr(a["lin0"], b["lin0"]))
            got["scalars"] = max(got["scalars"], lm_ref.relerr(a["lin1"], b["lin1"]), lm_ref.relerr(a["new1"], b["new1"]))
            got["state"] = max(got["state"], relerr(a["state"][0], b["state"][0]))
        print(f"{name}, {which}: trials {''.join(t['outcome'] for t in log['trials'])}; differences from the dense CPU loop {got}; "
              f"floor {floor}; tolerance {tol}")
        assert all(got[k] <= tol[k] for k in tol), (which, got, tol)
        assert log["lin_intact"]


def test_the_false_closure_is_survived_on_the_long_path(gpu, oracle):
    """test_between_gpu.py's false loop closure with all three closures long: Cauchy ends centimetres from the truth where
    the Gaussian model ends metres off, as on the widened band."""
    truth, init, G, priors = cr.lm_case("false-closure-cauchy")
    n, off = len(init), {}
    for name, loss in (("gauss", (0, 0.0)), ("cauchy", (2, 1.0))):
        Gk = br.BetweenSet(G.i, G.j, G.meas, 1.0 / G.w, [(0, 0.0)] * (n - 1) + [loss] * 3)
        prob, sv = pose_only(Gk, priors, n, max_span=cr.LM_MAX_SPAN)
        poses, _, rep = sv.optimize(d(init), no_points())
        off[name] = np.abs(poses.cpu().numpy()[:, 9:] - truth[:, 9:]).max()
    print(off)
    assert off["cauchy"] < 0.05 * off["gauss"] and off["gauss"] > 1.0


# ---- band, storage, defaults ---------------------------------------------------------------------------------------------
def test_band_storage_and_band_mode_are_those_of_the_graph_without_closures(gpu, oracle):
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    seq, span, far = stereo_200()
    n, nL = 200, len(seq["points_gt"])
    rng = np.random.default_rng(50)
    odo = [(i - 1, i) for i in range(1, n)]
    state = (d(seq["poses_init"]), d(seq["points_init"]))
    modes = {}
    for which, pairs, max_span in (("closures", odo + far[:3], span), ("none", odo, None)):
        G = measured(rng, seq["poses_gt"], pairs, 0.01)
        bf = device_set(G, n, max_span=max_span)
        prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n, nL, seq["K"], seq["sigma"], prior_pose=[0],
                               prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None], between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        assert prob.band == span and sv.Sband.shape[1] == span + 1 and not sv.use_split
        trial(sv, state)
        modes[which] = _lib.load().vus_ba_get_tuning(_lib.TUNE_LAST_BAND_MODE)
    assert modes["closures"] == modes["none"], modes


def test_defaults_take_todays_path(gpu, oracle):
    truth, init, G, priors = cr.lm_case("closure-40")
    n = len(init)
    prob0, sv0 = pose_only(G, priors, n)
    assert sv0.C is None and not hasattr(sv0, "clo_scal") and sv0._trial.numel() == 5 + 4 and "closure" not in sv0._families
    prob1, sv1 = pose_only(G, priors, n, max_span=G.span)           # nothing is longer: an empty long set
    assert sv1.C is None and sv1.B.long is None and prob1.band == prob0.band and sv1._trial.numel() == sv0._trial.numel()
    out = [sv.optimize(d(init), no_points()) for sv in (sv0, sv1)]
    assert out[0][2].lambda_hist == out[1][2].lambda_hist and out[0][2].long_closures == 0
    # the one-sided solve is deterministic up to the atomics of its back-substitution
    assert relerr(out[1][0].cpu().numpy(), out[0][0].cpu().numpy()) <= 1e-13
    prob2, sv2 = pose_only(G, priors, n, max_span=cr.LM_MAX_SPAN)
    assert sv2._trial.numel() == 5 + 4 * 2 and sv2.clo_scal.numel() == 4


# ---- the gtsam shim and run_sequence ---------------------------------------------------------------------------------------
def test_gtsam_set_long_closure_span(gpu, oracle):
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    truth, init, G, priors = cr.lm_case("closure-40")
    n = len(init)
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(priors[1][0]), gtsam.noiseModel.Diagonal.Sigmas(1.0 / priors[2][0])))
    for f in range(len(G.i)):
        graph.add(gtsam.BetweenFactorPose3(X(int(G.i[f])), X(int(G.j[f])), gtsam.Pose3.from_flat12(G.meas[f]),
                                           gtsam.noiseModel.Diagonal.Sigmas(1.0 / G.w[f])))
    assert (int(G.i[-1]), int(G.j[-1])) == (0, n - 1)
    for k in range(n):
        values.insert(X(k), gtsam.Pose3.from_flat12(init[k]))
    out = {}
    for m in (None, cr.LM_MAX_SPAN):
        prm = gtsam.LevenbergMarquardtParams()
        assert prm.getLongClosureSpan() is None
        prm.setLongClosureSpan(m)
        opt = gtsam.LevenbergMarquardtOptimizer(graph, values, prm)
        res = opt.optimize()
        out[m] = np.stack([res.atPose3(X(k)).flat12() for k in range(n)])
        assert opt.report().long_closures == (1 if m else 0)
    assert relerr(out[cr.LM_MAX_SPAN], out[None]) <= 1e-8


def test_run_sequence_with_long_span(gpu):
    """The rendered closed track of tests/loop_scene.py through run_sequence, the revisit X(0)-X(9) in the band (default)
    and as a long closure: the same last-keyframe error to 1e-6 m, and stages names the long set's size."""
    import loop_scene as S
    from visual_underwater_slam_amd import sequence, synth
    from visual_underwater_slam_amd.frontend import ImageProcessorParams
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    gt = S.poses_gt()
    frames = synth.scene_frames(gt, S.H, S.W, xp=torch, device="cuda").contiguous()
    init = S.poses_drifted(gt)
    # inertial data of straight legs at constant velocity between the keyframes (0.2 s apart): gravity alone on the
    # accelerometer of the z-down body, the track's even yaw rate on the gyro, the leg's velocity on the DVL
    T, n_per = 0.2, 40
    rate = S.YAW_END / (S.N_KF - 1) / T
    imu = [np.tile(np.array([0.0, 0.0, -synth.GRAVITY, 0.0, 0.0, -rate]), (n_per, 1)) for _ in range(S.N_KF - 1)]
    vel = np.diff(gt[:, 9:], axis=0) / T
    dvl = np.stack([gt[k, :9].reshape(3, 3).T @ vel[min(k, S.N_KF - 2)] for k in range(S.N_KF)])
    prm = ImageProcessorParams(max_features=S.KP, **sequence.SEQUENCE_PARAMS)
    last, stages = {}, {}
    for m in (None, 6):
        lc = sequence.LoopClosureParams(long_span=m)
        res, seq, st = sequence.run_sequence(frames, init, imu, dvl, disparity_sign=1, params=prm, loop_closure=lc)
        pairs = list(zip(*(x.tolist() for x in st["loop_pairs"])))
        assert S.REVISIT in pairs and st["loop_accepted"][pairs.index(S.REVISIT)]
        last[m] = res.atPose3(X(S.N_KF - 1)).translation()
        assert ("long_closures" in st) == (m is not None)          # the default run's stages are what they were
        stages[m] = st.get("long_closures", seq.optimizer.report().long_closures)
        print(f"long_span={m}: last keyframe {1e3 * np.linalg.norm(last[m] - gt[-1, 9:]):.2f} mm from the truth, "
              f"{stages[m]} long closures of {int(st['loop_accepted'].sum())} accepted")
    assert stages[None] == 0 and stages[6] >= 1
    assert np.linalg.norm(last[6] - last[None]) <= 1e-6


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, oracle):
    from visual_underwater_slam_amd import dist
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    truth, init, G, priors = cr.lm_case("closure-40")
    n = len(init)
    prob, sv = pose_only(G, priors, n, max_span=cr.LM_MAX_SPAN)
    with pytest.raises(NotImplementedError, match="long closures"):
        sv.marginals(d(init), no_points())
    rng = np.random.default_rng(60)
    many = measured(rng, truth, [(k - 1, k) for k in range(1, n)] + [(k % 10, 20 + k % 19) for k in range(65)], 0.01)
    with pytest.raises(ValueError, match="max_span.*fewer closures"):
        device_set(many, n, max_span=cr.LM_MAX_SPAN)
    widest = int(np.abs(many.i - many.j).max())
    assert device_set(many, n, max_span=widest).long is None and device_set(many, n).span == widest
    z = np.zeros((0,))
    prob2 = StereoBAProblem(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                            prior_pose=priors[0], prior_T=priors[1], prior_sigmas=1.0 / priors[2], between_span=1, pose_stride=2)
    with pytest.raises(ValueError, match="another problem"):
        StereoBASolver(prob2, device_set(G, n, 1, max_span=cr.LM_MAX_SPAN))
    with pytest.raises(ValueError, match="inside the problem's band"):      # the band reaches further than max_span
        StereoBASolver(pose_only(G, priors, n)[0], device_set(G, n, max_span=cr.LM_MAX_SPAN))
    with pytest.raises(NotImplementedError, match="landmark-sharded"):
        dist.ShardedStereoBASolver(z.astype(np.int32), z.astype(np.int32), np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0,
                                   between=device_set(G, n, max_span=cr.LM_MAX_SPAN))
