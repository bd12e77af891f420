"""BetweenFactorPose3 without a GPU: the numpy reference (residual, Jacobians, dense LM), the host CSR of the between blocks,
the Pose3 tangent-space helpers of the shim, the shim's factor and its lowering, and the refusals."""
import numpy as np
import pytest

import between_ref as br
from visual_underwater_slam_amd import gtsam
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L


def _pose(rng, scale=1.0):
    return gtsam.Pose3.Expmap(scale * rng.standard_normal(6))


def test_pose3_tangent_helpers_round_trip():
    rng = np.random.default_rng(0)
    for _ in range(20):
        T, xi = _pose(rng, 2.0), 0.7 * rng.standard_normal(6)
        assert np.allclose(T.localCoordinates(T.retract(xi)), xi, atol=1e-12)
        assert np.allclose(gtsam.Pose3.Logmap(gtsam.Pose3.Expmap(xi)), xi, atol=1e-12)
        # Expmap of a pure rotation is Rot3.Expmap; of a pure translation, the translation
        assert np.allclose(gtsam.Pose3.Expmap(np.r_[xi[:3], 0, 0, 0]).rotation().matrix(), gtsam.Rot3.Expmap(xi[:3]).matrix())
        assert np.allclose(gtsam.Pose3.Expmap(np.r_[0, 0, 0, xi[3:]]).translation(), xi[3:])
    assert np.allclose(gtsam.Pose3.Logmap(gtsam.Pose3()), 0.0)


def test_pose3_helpers_match_the_oracle_chart(oracle):
    rng = np.random.default_rng(1)
    for _ in range(10):
        T, xi = _pose(rng), 0.5 * rng.standard_normal(6)
        assert np.allclose(T.retract(xi).flat12(), oracle.pose_retract(T.flat12(), xi), atol=1e-13)
        T2 = _pose(rng)
        assert np.allclose(T.localCoordinates(T2), oracle.pose_local(T.flat12(), T2.flat12()), atol=1e-12)


def test_jacobians_match_central_differences(oracle):
    rng = np.random.default_rng(2)
    h = 1e-6
    for _ in range(5):
        T1, T2 = _pose(rng).flat12(), _pose(rng).flat12()
        M = br.flat_mul(br.flat_inv(T1), T2)
        M = oracle.pose_retract(M, 0.05 * rng.standard_normal(6))     # a measurement near, not at, the estimate
        H1, H2 = br.jacobians(T1, T2)
        # the Jacobians of Between (hx = T1^-1 T2) in the T Exp chart; the residual Log(M^-1 hx) adds d Local, which
        # GTSAM's default factor does not apply: compare the chart of hx itself
        hx = br.flat_mul(br.flat_inv(T1), T2)
        N1, N2 = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            e = np.zeros(6); e[k] = h
            for N, which in ((N1, 0), (N2, 1)):
                p = [T1, T2]; m = [T1, T2]
                p[which] = oracle.pose_retract(p[which], e)
                m[which] = oracle.pose_retract(m[which], -e)
                hp = br.flat_mul(br.flat_inv(p[0]), p[1])
                hm = br.flat_mul(br.flat_inv(m[0]), m[1])
                N[:, k] = (oracle.pose_local(hx, hp) - oracle.pose_local(hx, hm)) / (2 * h)
        assert np.allclose(H1, N1, atol=1e-7), np.abs(H1 - N1).max()
        assert np.allclose(H2, N2, atol=1e-7), np.abs(H2 - N2).max()
        r = br.residual(oracle, T1, T2, M)
        assert np.abs(r).max() < 0.5


def test_residual_is_zero_at_the_measurement_and_swapped_keys_give_the_same_error(oracle):
    rng = np.random.default_rng(3)
    T1, T2 = _pose(rng).flat12(), _pose(rng).flat12()
    M = br.flat_mul(br.flat_inv(T1), T2)
    assert np.abs(br.residual(oracle, T1, T2, M)).max() < 1e-12
    poses = np.stack([T1, T2])
    # swapped keys, inverted measurement: r' = Log(M hx^-1) = -Ad(M) r.  Ad(M) preserves the norm when M is a pure
    # rotation, so the error is the same under a rotation-isotropic, translation-isotropic weight
    Mr = np.concatenate([gtsam.Rot3.Expmap(0.4 * rng.standard_normal(3)).matrix().reshape(-1), np.zeros(3)])
    w = np.array([[2.0, 2.0, 2.0, 0.5, 0.5, 0.5]])
    G = br.BetweenSet([0], [1], Mr[None], 1.0 / w)
    Gs = br.BetweenSet([1], [0], br.flat_inv(Mr)[None], 1.0 / w)
    e, es = br.error(oracle, G, poses), br.error(oracle, Gs, poses)
    assert e > 0.01 and abs(e - es) <= 1e-12 * e
    r, rs = br.residual(oracle, T1, T2, Mr), br.residual(oracle, T2, T1, br.flat_inv(Mr))
    assert np.allclose(rs, -br.adjoint(Mr) @ r, atol=1e-12)


def test_dense_lm_recovers_a_noise_free_pose_graph_loop(oracle):
    rng = np.random.default_rng(4)
    truth, init, G, priors = br.pose_graph(rng, 20, closures=[(0, 19), (3, 15), (5, 12)])
    poses, _, rep = br.lm_optimize(oracle, G, init, priors=priors)
    assert rep["status"] == 0 and rep["final_error"] < 1e-12
    assert np.abs(poses - truth).max() < 1e-6


def test_between_targets_csr():
    from visual_underwater_slam_amd.ba import between_targets
    n1, n2 = np.array([0, 4, 2, 2]), np.array([1, 2, 4, 3])
    tn, ts, tp, tt = between_targets(n1, n2)
    blocks = {(int(a), int(b)): list(tt[tp[q]:tp[q + 1]]) for q, (a, b) in enumerate(zip(tn, ts))}
    assert list(zip(tn.tolist(), ts.tolist())) == sorted(blocks)
    assert blocks[(0, 0)] == [0] and blocks[(1, 0)] == [1] and blocks[(1, 1)] == [3]
    assert blocks[(4, 0)] == [4 * 1 + 0, 4 * 2 + 1]                  # factor 1 key1 = node 4, factor 2 key2 = node 4
    assert blocks[(2, 0)] == [4 * 1 + 1, 4 * 2 + 0, 4 * 3 + 0]
    assert blocks[(4, 2)] == [4 * 1 + 2, 4 * 2 + 3]                  # node1 > node2: J1^T J2; node2 > node1: transpose
    assert blocks[(3, 1)] == [4 * 3 + 3] and blocks[(3, 0)] == [4 * 3 + 1]
    assert tp[-1] == 3 * len(n1)


def _graph(n=6, closures=((0, 5),), robust=None):
    rng = np.random.default_rng(5)
    truth, init, G, priors = br.pose_graph(rng, n, closures=closures)
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(truth[0]), gtsam.noiseModel.Isotropic.Sigma(6, 1e-3)))
    noise = gtsam.noiseModel.Diagonal.Sigmas(1.0 / G.w[0])
    for f in range(len(G.i)):
        model = noise if robust is None or f < n - 1 else gtsam.noiseModel.Robust.Create(robust, noise)
        graph.add(gtsam.BetweenFactorPose3(X(int(G.i[f])), X(int(G.j[f])), gtsam.Pose3.from_flat12(G.meas[f]), model))
    for k in range(n):
        values.insert(X(k), gtsam.Pose3.from_flat12(init[k]))
    return graph, values, G


def test_shim_factor_construction_and_dimension_check():
    m = gtsam.Pose3(gtsam.Rot3.Rz(0.3), [1.0, 0.0, 0.0])
    f = gtsam.BetweenFactorPose3(X(1), X(2), m, gtsam.noiseModel.Unit.Create(6))
    assert f.keys() == [X(1), X(2)] and f.measured().equals(m) and f.noiseModel().dim() == 6
    assert "BetweenFactorPose3" in gtsam.__all__
    with pytest.raises(RuntimeError, match="6-dimensional"):
        gtsam.BetweenFactorPose3(X(1), X(2), m, gtsam.noiseModel.Isotropic.Sigma(3, 1.0))
    with pytest.raises(ValueError, match="both keys"):
        gtsam.BetweenFactorPose3(X(1), X(1), m, gtsam.noiseModel.Unit.Create(6))


def test_shim_lowering_without_a_gpu():
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    graph, values, G = _graph(closures=((0, 5), (4, 1)), robust=gtsam.noiseModel.mEstimator.Cauchy.Create(1.0))
    pg = _pack_graph(graph, values, device=None)
    b = pg["between"]
    assert b["i"].tolist() == G.i.tolist() and b["j"].tolist() == G.j.tolist()
    assert np.allclose(b["meas"], G.meas) and np.allclose(b["sigmas"], 1.0 / G.w)
    assert b["span"] == 5
    assert b["losses"][:5] == [(0, 0.0)] * 5 and b["losses"][5] == (2, 1.0)
    assert pg["prior_idx"].tolist() == [0]


def test_band_span_of_a_lowered_graph():
    """The between span that StereoBAProblem(between_span=...) widens the band by: the widest pose distance."""
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    graph, values, _ = _graph(n=12, closures=((0, 3), (11, 2)))
    assert _pack_graph(graph, values, device=None)["between"]["span"] == 9
    G = br.BetweenSet([0, 7, 2], [1, 2, 9], np.zeros((3, 12)), np.ones((3, 6)))
    assert G.span == 7


def test_refusals():
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    graph, values, _ = _graph()
    graph.add(gtsam.BetweenFactorPose3(X(0), X(99), gtsam.Pose3(), gtsam.noiseModel.Unit.Create(6)))
    with pytest.raises(RuntimeError, match="does not exist"):
        _pack_graph(graph, values, device=None)
    graph, values, _ = _graph()
    values.insert(L(0), np.zeros(3))
    graph.add(gtsam.BetweenFactorPose3(X(0), L(0), gtsam.Pose3(), gtsam.noiseModel.Unit.Create(6)))
    with pytest.raises(RuntimeError, match="does not exist"):          # a Point3 key is not a Pose3
        _pack_graph(graph, values, device=None)
    from visual_underwater_slam_amd import dist
    with pytest.raises(NotImplementedError, match="BetweenFactorPose3"):
        dist.ShardedStereoBASolver([0], [0], np.zeros((1, 3)), 1, 1, np.ones(6), 1.0, between=object())
