"""PriorFactorPoint3 on observed landmarks without a GPU: the numpy reference (tests/point_prior_ref.py) against central
differences of its own error, the packer's routing of landmark priors (observed -> pg["point_priors"], unobserved ->
the host aux path), the constructor's refusals and the host-side CSR of ba.PointPriors."""
import numpy as np
import pytest

import visual_underwater_slam_amd.gtsam as gtsam
from visual_underwater_slam_amd.gtsam import optimizer
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
import mono_problem
import point_prior_ref as ppr


def _reference(seq, single_lm):
    """PointPriorBA on the raw rows of seq (no oracle: only the prior term is used here)"""
    pk = {"n_poses": len(seq["poses_gt"]), "n_points": len(seq["points_gt"]), "n_obs": len(seq["meas"]),
          "obs_pose": seq["obs_pose"], "obs_point": seq["obs_point"], "meas": seq["meas"]}
    return ppr.PointPriorBA(None, pk, seq["K"], seq["sigma"], 0, 0.0, None, seq["mono"], seq["mono_K"], seq["mono_sigma"],
                            point_priors=ppr.prior_set(seq, single_lm))


def test_prior_blocks_against_central_differences_of_the_error():
    """gl and the Gauss-Newton block of every prior-carrying landmark against first and second central differences of the
    landmark's own prior error.  The error is quadratic, so the differences are exact at any step up to round-off (about
    eps x error / h^2 with h = 1, far below 1e-9 of the smallest entry here); the blocks are diagonal."""
    seq, single_lm = ppr.single_sighting(mono_problem.mixed_sequence(n_kf=16, n_lm=80))
    R = _reference(seq, single_lm)
    points = seq["points_init"]
    V, gl = R.prior_blocks(points)
    carrying = sorted(set(R.pp_idx.tolist()))
    assert carrying == sorted({0, 79, ppr.TRIPLE_LM, ppr.FAR_LM, ppr.STEREO_LM, single_lm})
    assert (R.pp_idx == ppr.TRIPLE_LM).sum() == 3
    h, E = 1.0, np.eye(3)
    for j in carrying:
        e = lambda p: R.prior_error_of(j, p)
        p = points[j]
        g = np.array([(e(p + h * E[k]) - e(p - h * E[k])) / (2 * h) for k in range(3)])
        H = np.array([[(e(p + h * E[a] + h * E[b]) - e(p + h * E[a] - h * E[b]) - e(p - h * E[a] + h * E[b])
                        + e(p - h * E[a] - h * E[b])) / (4 * h * h) for b in range(3)] for a in range(3)])
        assert np.allclose(gl[j], g, rtol=1e-9, atol=0), (j, gl[j], g)
        assert np.allclose(V[j, [0, 3, 5]], np.diag(H), rtol=1e-9, atol=0), (j, V[j], H)
        assert np.abs(H - np.diag(np.diag(H))).max() <= 1e-9 * np.diag(H).min() and not V[j, [1, 2, 4]].any()
    others = np.setdiff1d(np.arange(80), carrying)
    assert not V[others].any() and not gl[others].any()
    assert R.prior_error(points) == pytest.approx(sum(R.prior_error_of(j, points[j]) for j in carrying), rel=1e-14)
    # the sum over three priors on one landmark, stated by hand
    sel = R.pp_idx == ppr.TRIPLE_LM
    assert np.allclose(V[ppr.TRIPLE_LM, [0, 3, 5]], (R.pp_w[sel] ** 2).sum(0), rtol=1e-15)
    # the step evaluation of a linear factor is exact
    dl = 0.01 * np.arange(240.0).reshape(80, 3)
    lin0 = R.prior_error(points)
    want = lin0 + float(np.sum(gl * dl)) + 0.5 * sum(float(dl[j] @ np.diag(V[j, [0, 3, 5]]) @ dl[j]) for j in carrying)
    assert R.prior_error(points + dl) == pytest.approx(want, rel=1e-12)


CAL = gtsam.Cal3_S2(1800.0, 1750.0, 2.5, 960.0, 540.0)
CAL_ST = gtsam.Cal3_S2Stereo(1827.0, 1827.6, 0.0, 968.9, 561.4, 0.063)
MODEL2 = gtsam.noiseModel.Isotropic.Sigma(2, 7.0)
MODEL3 = gtsam.noiseModel.Isotropic.Sigma(3, 10.0)


def _values():
    v = gtsam.Values()
    for i in range(3):
        v.insert(X(i), gtsam.Pose3())
    for j in (0, 1, 2, 3, 9):
        v.insert(L(j), np.array([0.1 * j, 0.0, 4.0]))
    return v


def _graph(as_block):
    """stereo and mono factors on L(0), L(1), L(3) -- packed landmark indices 0, 1, 2; L(2) and L(9) are observed by none"""
    g = gtsam.NonlinearFactorGraph()
    g.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3(), gtsam.noiseModel.Isotropic.Sigma(6, 0.1)))
    pk, lk = [X(0), X(1), X(2)], [L(0), L(3), L(3)]
    uv = np.array([[100.0 + a, 200.0 + a] for a in range(3)])
    if as_block:
        g.push_back(gtsam.StereoFactorBlock([[50.0, 40.0, 60.0]], MODEL3, [X(1)], [L(1)], CAL_ST))
        g.push_back(gtsam.ProjectionFactorBlock(uv, MODEL2, pk, lk, CAL))
    else:
        g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(50.0, 40.0, 60.0), MODEL3, X(1), L(1), CAL_ST))
        for a in range(3):
            g.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(*uv[a]), MODEL2, pk[a], lk[a], CAL))
    return g


@pytest.mark.parametrize("as_block", (False, True))
def test_packer_routes_priors_on_observed_landmarks_to_the_gpu(as_block):
    g = _graph(as_block)
    diag = gtsam.noiseModel.Diagonal.Sigmas(np.array([0.05, 0.7, 5.0]))
    g.add(gtsam.PriorFactorPoint3(L(3), np.array([1.0, 2.0, 3.0]), diag))
    g.add(gtsam.PriorFactorPoint3(L(0), np.array([4.0, 5.0, 6.0]), gtsam.noiseModel.Isotropic.Sigma(3, 0.2)))
    g.add(gtsam.PriorFactorPoint3(L(9), np.array([0.0, 0.0, 1.0]), gtsam.noiseModel.Unit.Create(3)))      # unobserved
    g.add(gtsam.PriorFactorVector(L(3), np.array([7.0, 8.0, 9.0]), gtsam.noiseModel.Isotropic.Sigma(3, 2.0)))
    pg = optimizer._pack_graph(g, _values(), device=None)
    assert list(pg["lm_keys"]) == [L(0), L(1), L(3)]
    pp = pg["point_priors"]
    assert pp["idx"].tolist() == [2, 0, 2]                      # graph order, indices into lm_keys
    assert np.array_equal(pp["mean"], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])
    assert np.array_equal(pp["sigmas"], [[0.05, 0.7, 5.0], [0.2, 0.2, 0.2], [2.0, 2.0, 2.0]])
    aux = pg["aux"]
    assert aux.keys == [L(9)] and np.array_equal(aux.prior[0], [0.0, 0.0, 1.0]) and np.array_equal(aux.w[0], [1.0, 1.0, 1.0])
    # without a landmark prior the entry is None and the aux path is as before
    g0 = _graph(as_block)
    g0.add(gtsam.PriorFactorPoint3(L(9), np.array([0.0, 0.0, 1.0]), gtsam.noiseModel.Unit.Create(3)))
    pg0 = optimizer._pack_graph(g0, _values(), device=None)
    assert pg0["point_priors"] is None and pg0["aux"].keys == [L(9)]


def test_packer_and_constructor_refusals():
    g = _graph(False)
    g.add(gtsam.PriorFactorVector(L(3), np.array([1.0, 2.0]), gtsam.noiseModel.Isotropic.Sigma(2, 1.0)))
    with pytest.raises(RuntimeError, match="3-vector"):
        optimizer._pack_graph(g, _values(), device=None)
    # the aux path keeps its refusal of several priors on one unobserved variable
    g = _graph(False)
    for _ in range(2):
        g.add(gtsam.PriorFactorPoint3(L(9), np.zeros(3), gtsam.noiseModel.Unit.Create(3)))
    with pytest.raises(NotImplementedError, match="several prior factors"):
        optimizer._pack_graph(g, _values(), device=None)
    with pytest.raises(RuntimeError, match="3-vector"):
        gtsam.PriorFactorPoint3(L(0), np.zeros(2), gtsam.noiseModel.Isotropic.Sigma(2, 1.0))
    with pytest.raises(RuntimeError, match="3-dimensional"):
        gtsam.PriorFactorPoint3(L(0), np.zeros(3), gtsam.noiseModel.Isotropic.Sigma(2, 1.0))
    rob = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(1.345), gtsam.noiseModel.Isotropic.Sigma(3, 1.0))
    with pytest.raises(Exception, match="[Rr]obust"):
        gtsam.PriorFactorPoint3(L(0), np.zeros(3), rob)
    f = gtsam.PriorFactorPoint3(L(0), [1.0, 2.0, 3.0], gtsam.noiseModel.Diagonal.Sigmas(np.array([1.0, 2.0, 3.0])))
    assert f.keys() == [L(0)] and np.array_equal(f.prior(), [1.0, 2.0, 3.0]) and isinstance(f, gtsam.PriorFactorVector)


def test_point_priors_host_csr():
    """ba.PointPriors sorts stably by landmark and builds its CSR with numpy before anything is uploaded"""
    from visual_underwater_slam_amd import ba
    idx = [7, 2, 7, 0, 9, 7, 2]
    order, row_point, row_ptr = ba.csr_rows(idx)
    assert order.tolist() == [3, 1, 6, 0, 2, 5, 4]              # graph order within one landmark
    assert row_point.tolist() == [0, 2, 7, 9] and row_ptr.tolist() == [0, 1, 3, 6, 7]
    assert row_point.dtype == np.int32 and row_ptr.dtype == np.int32
    mean = np.arange(21.0).reshape(7, 3)
    sig = 1.0 + np.arange(21.0).reshape(7, 3)
    Q = ba.PointPriors(idx, mean, sig, 10, device="cpu")
    assert (Q.n, Q.n_points, Q.n_rows) == (7, 10, 4) and (Q.c.n, Q.c.n_points, Q.c.n_rows) == (7, 10, 4)
    assert np.array_equal(Q.host["idx"], [0, 2, 2, 7, 7, 7, 9]) and np.array_equal(Q.host["mean"], mean[order])
    assert np.array_equal(Q.mean.numpy(), mean[order]) and np.array_equal(Q.w.numpy(), 1.0 / sig[order])
    assert Q.row_point.tolist() == [0, 2, 7, 9] and Q.row_ptr.tolist() == [0, 1, 3, 6, 7] and Q.addr()
    empty = ba.PointPriors([], np.zeros((0, 3)), np.zeros((0, 3)), 10, device="cpu")
    assert (empty.n, empty.n_rows) == (0, 0) and empty.c.row_point is None and empty.c.w is None
    assert ba.csr_rows([])[2].tolist() == [0]
    for bad in (dict(point_idx=[0, 10]), dict(point_idx=[-1, 0]), dict(mean=np.zeros((3, 3))), dict(sigmas=np.zeros((2, 3))),
                dict(sigmas=np.full((2, 3), np.inf)), dict(sigmas=-np.ones((2, 3))), dict(mean=np.full((2, 3), np.nan))):
        kw = dict(point_idx=[0, 1], mean=np.zeros((2, 3)), sigmas=np.ones((2, 3)), n_points=10, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError, match="point priors"):
            ba.PointPriors(**kw)
