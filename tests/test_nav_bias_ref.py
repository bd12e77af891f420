"""CPU checks of the per-keyframe-bias graph (NavBiasBASolver): the dense reference of nav_bias_ref.py that the GPU tests
compare against (its gradient is the derivative of the total error, A is symmetric positive definite, one LM step is the
dense solve retracted, a stiff bias random walk reproduces the shared-bias oracle LM), the host-side validation of the
vus_navb_* entry points, and the gtsam shim's packing, key mapping and refusals."""
import ctypes

import numpy as np
import pytest

from visual_underwater_slam_amd import synth
from test_nav_oracle import build_nav
import nav_bias_ref as nbr


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _state(s, seed=4):
    rng = np.random.default_rng(seed)
    n = len(s["poses_gt"])
    return s["poses_init"], s["vels_gt"] + 0.05 * rng.normal(size=(n, 3)), 0.01 * rng.normal(size=(n, 6)), s["points_init"]


def test_gradient_is_the_derivative_of_the_total_error(oracle):
    s = synth.nav_sequence(6, 120, 30, bias_walk_sigma=(2e-3, 2e-4))
    P, G = nbr.make_graph(oracle, s)
    poses, vels, biases, points = _state(s)
    n = len(poses)
    ref = nbr.dense_system(oracle, s, P, G, poses, vels, biases, points, 0.0)
    assert np.isclose(ref["err"], nbr.total_error(oracle, P, G, poses, vels, biases, points), rtol=1e-12)
    total = lambda *st: nbr.total_error(oracle, P, G, *st)
    h = 1e-6
    fd = lambda pert: (total(*pert(h)) - total(*pert(-h))) / (2 * h)
    dp, dv, pad, db = nbr.split_step(ref["gcam"], n)
    assert not pad.any()
    fd_p, fd_v, fd_b = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros((n, 6))
    for i in range(n):
        for k in range(6):
            def pp(t, i=i, k=k):
                xi = np.zeros(6); xi[k] = t
                q = poses.copy(); q[i] = oracle.pose_retract(poses[i], xi)
                return q, vels, biases, points
            fd_p[i, k] = fd(pp)

            def pb(t, i=i, k=k):
                b = biases.copy(); b[i, k] += t
                return poses, vels, b, points
            fd_b[i, k] = fd(pb)
        for k in range(3):
            def pv(t, i=i, k=k):
                v = vels.copy(); v[i, k] += t
                return poses, v, biases, points
            fd_v[i, k] = fd(pv)
    scale = np.abs(ref["gcam"]).max()
    for got, want, name in ((dp, fd_p, "pose"), (dv, fd_v, "velocity"), (db, fd_b, "bias")):
        assert np.abs(got - want).max() < 1e-6 * scale, (name, np.abs(got - want).max() / scale)
    # every bias coordinate carries gradient from its ImuFactor and its bias factors
    assert (np.abs(db[:-1]) > 0).all()


def test_matrix_is_symmetric_positive_definite_and_banded(oracle):
    s = synth.nav_sequence(8, 160, 40, bias_walk_sigma=(2e-3, 2e-4))
    P, G = nbr.make_graph(oracle, s)
    ref = nbr.dense_system(oracle, s, P, G, *_state(s), 0.0)
    A, n = ref["A"], 8
    assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()
    assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
    for i in range(n):              # velocity padding: decoupled unit rows
        r = 6 * (3 * i + 1) + 3
        assert np.array_equal(A[r:r + 3], np.eye(len(A))[r:r + 3])
    # the inertial blocks reach 4 nodes, the stereo ones 3 * (pose band)
    Hn = ref["Hnav"]
    for a in range(3 * n):
        for b in range(a + 5, 3 * n):
            assert not Hn[6 * b:6 * b + 6, 6 * a:6 * a + 6].any(), (a, b)
    assert Hn[6 * 4:6 * 5, 0:6].any()                  # X(0) .. V(1): 4 nodes apart
    assert Hn[6 * 5:6 * 6, 6 * 2:6 * 3].any()          # B(0) .. B(1): the between-factor


def test_first_lm_step_equals_the_dense_solve(oracle):
    s = synth.nav_sequence(8, 160, 40, bias_walk_sigma=(2e-3, 2e-4))
    P, G = nbr.make_graph(oracle, s)
    n = 8
    poses, vels, biases, points = s["poses_init"], np.zeros((n, 3)), np.zeros((n, 6)), s["points_init"]
    lam = oracle.LM_DEFAULTS["lambda_initial"]
    op, ov, ob, opt, rep = nbr.lm_optimize(oracle, s, P, G, poses, vels, biases, points, max_iterations=1)
    assert (rep["tries"], rep["iterations"]) == (1, 1)
    ref = nbr.dense_system(oracle, s, P, G, poses, vels, biases, points, lam)
    x, kappa, _ = nbr.solve(ref["A"], -ref["g"])
    np_, nv, nb = nbr.retract(oracle, poses, vels, biases, x)
    tol = max(1e-10, kappa * 2.2e-16)
    assert relerr(np_, op) < tol and relerr(nv, ov) < tol and relerr(nb, ob) < tol
    assert not nbr.split_step(x, n)[2].any()
    dl = oracle.ba_backsub(P, ref["lin"], ref["sch"]["Vinv"], nbr.split_step(x, n)[0])
    assert relerr(points + dl, opt) < tol
    assert rep["final_error"] < rep["initial_error"]


# A stiff random walk forces every bias onto one value: the per-keyframe solve then converges to the shared-bias
# solution.  Both LMs run to a tight tolerance (1e-12) so that what remains is the model difference: a walk of sigma s per
# sqrt(second) lets neighbouring biases differ by ~s, which moves the optimum by O(s^2).  Measured (8 keyframes, weak
# prior sigma 1e3 on B(0), which the shared-bias graph lacks), relative differences at s = 1e-4 / 1e-5 / 1e-6:
#   final error 1.73e-5 / 1.73e-7 / 1.66e-9   (= 1.7e3 s^2)      poses 3.8e-6 / 3.8e-8 / 6.9e-9  (3.8e2 s^2 + round-off)
#   velocities  1.71e-5 / 1.71e-7 / 6.9e-9    (1.7e3 s^2)        biases 7.8e-4 / 7.2e-6 / 8.0e-7
# At s = 1e-7 the between-factors' weight (5e14) makes the system's round-off dominate (poses 1.9e-7).  The test runs at
# s = 1e-5 with bounds of 3x the measured s^2 law: error 5e3 s^2, poses 1.2e3 s^2, velocities 5e3 s^2, biases 2.2e-5.
STIFF_S = 1e-5


def test_stiff_bias_walk_reproduces_the_shared_bias_oracle(oracle):
    s = synth.nav_sequence(8, 160, 40)
    P, G = nbr.make_graph(oracle, s, rw_sigma=(STIFF_S, STIFF_S), bias_prior_sigma=(1e3, 1e3))
    Ps, N = build_nav(oracle, s)
    poses, vels, points = s["poses_init"], np.zeros((8, 3)), s["points_init"]
    tight = dict(rel_tol=1e-12, abs_tol=1e-12)
    sp, sv, sb, spt, srep = oracle.nav_lm_optimize(Ps, N, poses, vels, np.zeros(6), points, **tight)
    kp, kv, kb, kpt, krep = nbr.lm_optimize(oracle, s, P, G, poses, vels, np.zeros((8, 6)), points, **tight)
    assert srep["status"] == 0 and krep["status"] == 0
    s2 = STIFF_S ** 2
    e = abs(krep["final_error"] - srep["final_error"]) / srep["final_error"]
    assert e < 5e3 * s2, e
    assert relerr(kp, sp) < 1.2e3 * s2 and relerr(kv, sv) < 5e3 * s2, (relerr(kp, sp), relerr(kv, sv))
    assert relerr(kb, np.broadcast_to(sb, kb.shape)) < 2.2e-5, relerr(kb, np.broadcast_to(sb, kb.shape))


# ---- host-side validation of the C ABI (no GPU: every case is refused before any device call) -----------------------
def _lib():
    from visual_underwater_slam_amd import _lib as L
    return L, L.load()


def test_header_is_separate_and_declares_the_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "vus_nav_bias.h")).read()
    for name in ("vus_navb_linearize", "vus_navb_assemble", "vus_navb_eval_step", "vus_navb_error", "vus_navb_work_doubles",
                 "vus_navb_factors"):
        assert name in txt
    vus = open(os.path.join(root, "include", "vus.h")).read()
    import re
    code = re.sub(r"/\*.*?\*/", "", vus, flags=re.S)       # test_abi's twin rule reads declarations of vus.h itself
    assert '#include "vus_nav_bias.h"' in code and "vus_navb_" not in code
    L, lib = _lib()
    for name in ("vus_navb_linearize", "vus_navb_assemble", "vus_navb_eval_step", "vus_navb_error"):
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from visual_underwater_slam_amd.ba import _CNavBias
    L, lib = _lib()
    B = ctypes.c_void_p(8)
    err = lambda: lib.vus_last_error().decode()
    N = _CNavBias()
    N.n_imu = 0
    addr = ctypes.addressof(N)
    # null buffers and a null factor set
    assert lib.vus_navb_linearize(addr, 4, None, B, B, B, B, B, B, None) == -1 and "null" in err()
    assert lib.vus_navb_linearize(None, 4, B, B, B, B, B, B, B, None) == -1 and "null" in err()
    assert lib.vus_navb_error(addr, 4, B, B, B, None, B, None) == -1 and "null" in err()
    assert lib.vus_navb_eval_step(addr, 4, B, B, B, B, B, B, None, B, B, None) == -1 and "null" in err()
    assert lib.vus_navb_assemble(12, 4, 0.0, B, None, B, B, None) == -1 and "null" in err()
    # sizes
    assert lib.vus_navb_error(addr, 0, B, B, B, B, B, None) == -1 and "n_poses" in err()
    N.n_bbetween = -1
    assert lib.vus_navb_error(addr, 4, B, B, B, B, B, None) == -1 and "bad sizes" in err()
    N.n_bbetween = 3
    assert lib.vus_navb_error(addr, 4, B, B, B, B, B, None) == -1 and "between" in err()     # arrays are null
    N.n_bbetween, N.n_bprior = 0, 1
    assert lib.vus_navb_error(addr, 4, B, B, B, B, B, None) == -1 and "prior" in err()
    N.n_bprior, N.n_imu = 0, 2
    assert lib.vus_navb_linearize(addr, 4, B, B, B, B, B, B, B, None) == -1 and "imu" in err()
    # the node count of the assembly: 3 nodes per keyframe, and the band the ImuFactors need
    assert lib.vus_navb_assemble(10, 4, 0.0, B, B, B, B, None) == -1 and "3 * n_poses" in err()
    assert lib.vus_navb_assemble(12, 3, 0.0, B, B, B, B, None) == -1 and "band" in err()
    assert lib.vus_navb_assemble(12, 12, 0.0, B, B, B, B, None) == -1 and "band" in err()
    assert lib.vus_navb_assemble(12, 4, -1.0, B, B, B, B, None) == -1 and "lambda" in err()
    assert lib.vus_navb_work_doubles(None) == 0


def test_nav_bias_factors_refuse_non_consecutive_links():
    from visual_underwater_slam_amd.ba import NavBiasFactors
    with pytest.raises(NotImplementedError, match="non-consecutive biases"):
        NavBiasFactors([0, 0, -9.81], bbetween=([0], [2], np.zeros((1, 6)), np.ones((1, 6))), device="cpu")
    with pytest.raises(NotImplementedError, match="non-consecutive poses"):
        NavBiasFactors([0, 0, -9.81], imu=([0], [2], np.zeros((1, 148)), np.zeros((1, 81))), device="cpu")
    f = NavBiasFactors([0, 0, -9.81], bbetween=([0, 1], [1, 2], np.zeros((2, 6)), np.ones((2, 6))),
                       bprior=([0], np.zeros((1, 6)), np.ones((1, 6))), device="cpu")
    assert list(f.unconstrained_biases(5)) == [3, 4] and list(f.unconstrained_biases(3)) == []


# ---- the gtsam shim --------------------------------------------------------------------------------------------------
def shim_graph(s, rw_sigma=(1e-2, 1e-3), n=None, dvl=True, robust_between=False):
    """A graph as a GTSAM user writes it (ImuFactorsExample): X(i), V(i), B(i) per keyframe, stereo factors, a pose
    prior, ImuFactor(.., B(i), pim), BetweenFactorConstantBias(B(i), B(i+1)), PriorFactorConstantBias(B(0)), DVL."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B, L
    n = len(s["poses_gt"]) if n is None else n
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    K = gtsam.Cal3_S2Stereo(*s["K"])
    noise = gtsam.noiseModel.Isotropic.Sigma(3, s["sigma"])
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(s["poses_gt"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(s["prior_sigmas"])))
    graph.add(gtsam.PriorFactorVector(V(0), np.zeros(3), gtsam.noiseModel.Isotropic.Sigma(3, 0.1)))
    graph.add(gtsam.PriorFactorConstantBias(B(0), gtsam.imuBias.ConstantBias(),
                                            gtsam.noiseModel.Diagonal.Sigmas(np.array([0.1] * 3 + [0.01] * 3))))
    params = gtsam.PreintegrationParams.MakeSharedU(9.81)
    params.setAccelerometerCovariance(nbr.ACC_COV); params.setGyroscopeCovariance(nbr.GYRO_COV)
    params.setIntegrationCovariance(nbr.INT_COV)
    dt = float(s["imu"][0, :, 6].sum()) if n > 1 else 0.2
    bsig = np.repeat(np.asarray(rw_sigma, float), 3) * np.sqrt(dt)
    bnoise = gtsam.noiseModel.Diagonal.Sigmas(bsig)
    if robust_between:
        bnoise = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(1.0), bnoise)
    for i in range(n):
        values.insert(X(i), gtsam.Pose3.from_flat12(s["poses_init"][i]))
        values.insert(V(i), np.zeros(3))
        values.insert(B(i), gtsam.imuBias.ConstantBias())
        if i == 0:
            continue
        pim = gtsam.PreintegratedImuMeasurements(params, gtsam.imuBias.ConstantBias())
        for smp in s["imu"][i - 1]:
            pim.integrateMeasurement(smp[:3], smp[3:6], smp[6])
        graph.add(gtsam.ImuFactor(X(i - 1), V(i - 1), X(i), V(i), B(i - 1), pim))
        graph.add(gtsam.BetweenFactorConstantBias(B(i - 1), B(i), gtsam.imuBias.ConstantBias(), bnoise))
        if dvl:
            graph.add(gtsam.DvlVelocityFactor(gtsam.noiseModel.Isotropic.Sigma(3, 0.1), V(i), X(i), s["dvl"][i]))
    keep = s["obs_pose"] < n
    lms = np.unique(s["obs_point"][keep])
    for j in lms:
        values.insert(L(int(j)), s["points_init"][j])
    for a in np.nonzero(keep)[0]:
        graph.add(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*s["meas"][a]), noise, X(int(s["obs_pose"][a])),
                                              L(int(s["obs_point"][a])), K))
    return graph, values


def test_shim_packs_the_per_keyframe_graph():
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import B, V
    s = synth.nav_sequence(6, 120, 30, bias_walk_sigma=(2e-3, 2e-4))
    graph, values = shim_graph(s)
    pg = _pack_graph(graph, values)
    nav = pg["nav"]
    assert nav["per_keyframe"] and nav["bias_key"] is None
    assert nav["bias_keys"] == [B(i) for i in range(6)] and nav["vel_keys"] == [V(i) for i in range(6)]
    assert nav["bias"].shape == (6, 6) and not nav["bias"].any()
    ii, jj, pims, Ws = nav["imu"]
    assert list(ii) == list(range(5)) and list(jj) == list(range(1, 6))
    pre, W = nbr.preintegrate(s)
    assert np.allclose(pims, pre, rtol=1e-12, atol=1e-18) and np.allclose(Ws, W, rtol=1e-9)
    bi, bj, bm, bs = nav["bbetween"]
    assert list(bi) == list(range(5)) and list(bj) == list(range(1, 6)) and not bm.any()
    assert np.allclose(bs, np.repeat([1e-2, 1e-3], 3) * np.sqrt(0.2))
    pi, pm, ps = nav["bprior"]
    assert list(pi) == [0] and not pm.any() and np.allclose(ps, [0.1] * 3 + [0.01] * 3)
    # a graph with one shared bias and no bias factors keeps the shared-bias layout
    from visual_underwater_slam_amd import gtsam
    g1 = gtsam.NonlinearFactorGraph()
    for f in graph._other:
        if isinstance(f, gtsam.ImuFactor):
            g1.add(gtsam.ImuFactor(*f._keys[:4], B(0), _pim_of(f)))
        elif not isinstance(f, (gtsam.PriorFactorConstantBias, gtsam.BetweenFactorConstantBias)):
            g1.add(f)
    nav1 = _pack_graph(_with_stereo(g1, graph), values)["nav"]
    assert not nav1["per_keyframe"] and nav1["bias_key"] == B(0) and nav1["bias"].shape == (6,)


def _pim_of(f):
    """A PreintegratedImuMeasurements stand-in carrying an existing ImuFactor's packed record."""
    class _Pre:
        dt = 1.0
    class _P:
        class params:
            use2ndOrderCoriolis = False
            omegaCoriolis = np.zeros(3)
            n_gravity = f.gravity
        _pre = _Pre()
    _P._pre.packed = lambda: f.pim
    _P._pre.whitening = lambda: f.W.reshape(9, 9)
    return _P


def _with_stereo(g, src):
    """g plus the stereo factors of src (recorded column-wise when they were added)."""
    from visual_underwater_slam_amd import gtsam
    m, pk, lk, model, K, _ = src._stereo_columns()
    for a in range(len(pk)):
        g.add(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*m[a]), model, int(pk[a]), int(lk[a]), K))
    return g


def _refused(graph, values, exc, match):
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    with pytest.raises(exc, match=match):
        _pack_graph(graph, values)


def test_shim_refuses_what_the_layout_cannot_hold():
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import B, X, V
    s = synth.nav_sequence(5, 100, 25)
    graph, values = shim_graph(s)
    # a missing B(i)
    v2 = gtsam.Values(values)
    v2.erase(B(3))
    _refused(graph, v2, RuntimeError, r"bias b3 of keyframe x3 is missing")
    # a non-consecutive bias between-factor
    g = _with_stereo(gtsam.NonlinearFactorGraph(), graph)
    for f in graph._other:
        g.add(f)
    g.add(gtsam.BetweenFactorConstantBias(B(0), B(2), gtsam.imuBias.ConstantBias(),
                                          gtsam.noiseModel.Isotropic.Sigma(6, 0.01)))
    _refused(g, values, NotImplementedError, r"BetweenFactorConstantBias\(b0, b2\): only consecutive")
    # an ImuFactor whose bias key is B(j), the later keyframe's
    g = _with_stereo(gtsam.NonlinearFactorGraph(), graph)
    for f in graph._other:
        if isinstance(f, gtsam.ImuFactor) and f._keys[0] == X(3):
            g.add(gtsam.ImuFactor(X(3), V(3), X(4), V(4), B(4), _pim_of(f)))
        else:
            g.add(f)
    _refused(g, values, NotImplementedError, r"uses the bias b4; with per-keyframe biases it must use b3")
    # one shared bias mixed with per-keyframe biases
    g = _with_stereo(gtsam.NonlinearFactorGraph(), graph)
    for f in graph._other:
        g.add(gtsam.ImuFactor(*f._keys[:4], B(0), _pim_of(f)) if isinstance(f, gtsam.ImuFactor) else f)
    _refused(g, values, NotImplementedError, r"mixes one shared bias \(b0 in 4 ImuFactors\)")
    # a robust model on a bias factor
    g2, v3 = shim_graph(s, robust_between=True)
    _refused(g2, v3, NotImplementedError, r"robust noise models on bias factors")
    # a bias factor on a key that is no keyframe's bias
    g = _with_stereo(gtsam.NonlinearFactorGraph(), graph)
    for f in graph._other:
        g.add(f)
    g.add(gtsam.PriorFactorConstantBias(B(9), gtsam.imuBias.ConstantBias(), gtsam.noiseModel.Isotropic.Sigma(6, 0.1)))
    _refused(g, values, NotImplementedError, r"on b9: not the bias B\(i\) of a keyframe")


def test_shim_maps_failing_nodes_to_keys():
    from visual_underwater_slam_amd.gtsam.marginals import Marginals
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import B, V, X
    m = Marginals.__new__(Marginals)
    m._lm_keys, m._pose_keys = [], [X(i) for i in range(4)]
    m._vel_keys, m._bias_keys, m._bias_key = [V(i) for i in range(4)], [B(i) for i in range(4)], None
    assert m._key_of("node", 0) == X(0) and m._key_of("node", 7) == V(2) and m._key_of("node", 11) == B(3)
    assert m._key_of("bias", 2) == B(2)
    m._bias_keys, m._bias_key = [], B(0)                  # the shared-bias layout is unchanged
    assert m._key_of("node", 3) == V(1) and m._key_of("bias", 0) == B(0)
