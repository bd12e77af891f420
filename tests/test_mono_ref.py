"""Monocular projection factors without a GPU: the numpy reference (tests/mono_ref.py) against finite differences, its
cheirality branch, and the gtsam-shaped names -- Point2, Cal3_S2, PinholeCameraCal3_S2, GenericProjectionFactorCal3_S2,
ProjectionFactorBlock -- with the graph's column-wise recording and every refusal of the packer."""
import numpy as np
import pytest

import visual_underwater_slam_amd.gtsam as gtsam
from visual_underwater_slam_amd.gtsam import optimizer
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
from visual_underwater_slam_amd import synth
import mono_ref
import sensor_ref

KM = np.array([1800.0, 1750.0, 2.5, 960.0, 540.0])       # nonzero skew
S = sensor_ref.extrinsic()


def _random_case(n, seed):
    """camera poses and points with z > 0 in the camera frame"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R = synth._rodrigues(rng.normal(0, 0.6, 3))
        t = rng.normal(0, 1.0, 3)
        q = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1.0, 6.0)])
        out.append((np.concatenate([R.reshape(9), t]), R @ q + t, rng.uniform(0, 1900, 2)))
    return out


def test_mono_jacobians_against_central_differences(oracle):
    h = 1e-6
    for T, p, m in _random_case(12, 1):
        r, H1, H2 = mono_ref.mono_factor(T, p, m, KM, 0.1)
        fd2 = np.stack([(mono_ref.mono_factor(T, p + h * e, m, KM, 0.1)[0] - mono_ref.mono_factor(T, p - h * e, m, KM, 0.1)[0]) / (2 * h)
                        for e in np.eye(3)], 1)
        fd1 = np.stack([(mono_ref.mono_factor(oracle.pose_retract(T, h * e), p, m, KM, 0.1)[0]
                         - mono_ref.mono_factor(oracle.pose_retract(T, -h * e), p, m, KM, 0.1)[0]) / (2 * h) for e in np.eye(6)], 1)
        scale = np.abs(H1).max()
        assert np.abs(H2 - fd2).max() <= 1e-6 * scale
        assert np.abs(H1 - fd1).max() <= 1e-6 * scale
        assert np.abs(H1).min(1).max() > 0 and H1[0, 1] != 0        # the skew reaches the u row


def _tiny_ba(oracle, sensor, poses, points, meas, is_mono):
    n = len(meas)
    pk = {"n_poses": len(poses), "n_points": len(points), "n_obs": n, "obs_pose": np.arange(n) % len(poses),
          "obs_point": np.arange(n) % len(points), "meas": meas}
    K = np.array([*synth.INTRINSIC[:2], 0.0, *synth.INTRINSIC[2:], synth.BASELINE_M])
    return mono_ref.MonoBA(oracle, pk, K, 10.0, 0, 0.0, sensor, is_mono, KM, 7.0)


@pytest.mark.parametrize("with_sensor", (False, True))
def test_mixed_factors_against_central_differences_in_the_body_tangent(oracle, with_sensor):
    """MonoBA.factors (mono rows in slots 0 and 2, stereo rows from the oracle, H1 in the BODY tangent) against central
    differences of its own residual through the oracle's retraction of the body pose"""
    sensor = S if with_sensor else None
    cases = _random_case(6, 2)
    cams = np.stack([c[0] for c in cases])
    poses = np.stack([sensor_ref.compose(c, sensor_ref.inverse(S)) for c in cams]) if with_sensor else cams
    points = np.stack([c[1] for c in cases])
    meas = np.stack([[c[2][0], np.nan if a % 2 == 0 else c[2][0] - 20.0, c[2][1]] for a, c in enumerate(cases)])
    is_mono = np.arange(6) % 2 == 0
    R = _tiny_ba(oracle, sensor, poses, points, meas, is_mono)
    r, H1, H2 = R.factors(poses, points)
    assert np.isfinite(r).all() and not r[is_mono, 1].any() and not H1[is_mono, 1].any() and not H2[is_mono, 1].any()
    assert np.abs(r[~is_mono, 1]).min() > 0
    h = 1e-6
    for a in range(6):
        for k in range(6):
            pp, pm = poses.copy(), poses.copy()
            pp[a] = oracle.pose_retract(poses[a], h * np.eye(6)[k])
            pm[a] = oracle.pose_retract(poses[a], -h * np.eye(6)[k])
            fd = (R.factors(pp, points)[0][a] - R.factors(pm, points)[0][a]) / (2 * h)
            assert np.abs(fd - H1[a][:, k]).max() <= 1e-6 * np.abs(H1[a]).max(), (a, k)
        for k in range(3):
            pp, pm = points.copy(), points.copy()
            pp[a, k] += h
            pm[a, k] -= h
            fd = (R.factors(poses, pp)[0][a] - R.factors(poses, pm)[0][a]) / (2 * h)
            assert np.abs(fd - H2[a][:, k]).max() <= 1e-6 * np.abs(H2[a]).max(), (a, k)


def test_cheirality_branch(oracle):
    T, p, m = _random_case(1, 3)[0]
    R, t = T[:9].reshape(3, 3), T[9:]
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    for pose, behind in ((T, R @ np.array([0.3, -0.2, -1e-3]) + t), (T, R @ np.array([0.3, -0.2, -2.0]) + t),
                         (eye, np.array([0.3, -0.2, 0.0]))):          # z = 0 exactly belongs to the branch
        r, H1, H2 = mono_ref.mono_factor(pose, behind, m, KM, 0.125)
        assert np.array_equal(r, np.full(2, 2.0 * KM[0] * 0.125)) and not H1.any() and not H2.any()
    # through MonoBA: rows 0 and 2 carry the constant, row 1 stays zero, d^2 is taken over two rows
    poses, points = T[None], (R @ np.array([0.3, -0.2, -2.0]) + t)[None]
    B = _tiny_ba(oracle, None, poses, points, np.array([[m[0], np.nan, m[1]]]), [1])
    r, H1, H2 = B.factors(poses, points)
    c = 2.0 * KM[0] * (1.0 / 7.0)          # whitened by w = 1 / sigma, as the kernels do
    assert np.array_equal(r[0], [c, 0.0, c]) and not H1.any() and not H2.any()
    assert B.error(poses, points) == pytest.approx(c * c, rel=1e-15)


def test_pinhole_camera_projects_what_the_factor_predicts():
    cal = gtsam.Cal3_S2(*KM)
    for T, p, m in _random_case(5, 4):
        cam = gtsam.PinholeCameraCal3_S2(gtsam.Pose3.from_flat12(T), cal)
        uv = cam.project(p)
        r, _, _ = mono_ref.mono_factor(T, p, m, KM, 0.25)
        assert np.allclose(r / 0.25 + m, uv, rtol=0, atol=1e-9)
        depth = (T[:9].reshape(3, 3).T @ (p - T[9:]))[2]
        assert np.allclose(cam.backproject(uv, depth), p, rtol=0, atol=1e-9)
        assert cam.pose().equals(gtsam.Pose3.from_flat12(T)) and cam.calibration() is cal
    T, p, _ = _random_case(1, 5)[0]
    behind = T[:9].reshape(3, 3) @ np.array([0.1, 0.1, -1.0]) + T[9:]
    with pytest.raises(RuntimeError, match="behind"):
        gtsam.PinholeCameraCal3_S2(gtsam.Pose3.from_flat12(T), cal).project(behind)


def test_point2_and_cal3_s2_accessors():
    assert np.array_equal(gtsam.Point2(1.5, -2.0), [1.5, -2.0]) and gtsam.Point2([3, 4]).dtype == float
    c = gtsam.Cal3_S2(*KM)
    assert (c.fx(), c.fy(), c.skew(), c.px(), c.py()) == tuple(KM)
    assert np.array_equal(c.vector(), KM)
    assert np.array_equal(c.K(), [[KM[0], KM[2], KM[3]], [0, KM[1], KM[4]], [0, 0, 1]])
    assert c.equals(gtsam.Cal3_S2(*KM)) and not c.equals(gtsam.Cal3_S2(*(KM + [0, 0, 1e-3, 0, 0])))


def _values(n_kf=3, n_lm=4):
    v = gtsam.Values()
    for i in range(n_kf):
        v.insert(X(i), gtsam.Pose3(gtsam.Rot3(), np.array([0.1 * i, 0.0, 0.0])))
    for j in range(n_lm):
        v.insert(L(j), np.array([0.1 * j, 0.0, 4.0]))
    return v


MODEL2 = gtsam.noiseModel.Isotropic.Sigma(2, 7.0)
MODEL3 = gtsam.noiseModel.Isotropic.Sigma(3, 10.0)
CAL = gtsam.Cal3_S2(*KM)
CAL_ST = gtsam.Cal3_S2Stereo(1827.0, 1827.6, 0.0, 968.9, 561.4, 0.063)


def test_projection_factor_constructor_and_accessors():
    Sp = gtsam.Pose3.from_flat12(S)
    f = gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(10.0, 20.0), MODEL2, X(1), L(2), CAL, Sp)
    assert f.keys() == [X(1), L(2)] and np.array_equal(f.measured(), [10.0, 20.0])
    assert f.calibration() is CAL and f.noiseModel() is MODEL2
    assert f.body_P_sensor().equals(Sp) and f.body_P_sensor() is not Sp
    assert gtsam.GenericProjectionFactorCal3_S2([1.0, 2.0], MODEL2, X(0), L(0), CAL).body_P_sensor() is None
    with pytest.raises(RuntimeError, match="2-dimensional"):
        gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(1, 2), MODEL3, X(0), L(0), CAL)
    with pytest.raises(RuntimeError, match="Cal3_S2"):
        gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(1, 2), MODEL2, X(0), L(0), CAL_ST)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        gtsam.ProjectionFactorBlock(np.zeros((2, 2)), MODEL3, [X(0), X(1)], [L(0), L(0)], CAL)
    with pytest.raises(RuntimeError, match="length"):
        gtsam.ProjectionFactorBlock(np.zeros((2, 2)), MODEL2, [X(0)], [L(0), L(0)], CAL)


def _mixed_graph(as_block, model2=MODEL2, model3=MODEL3, mono_sensor=None, stereo_sensor=None):
    g = gtsam.NonlinearFactorGraph()
    uv = np.array([[100.0 + a, 200.0 + a] for a in range(4)])
    pk, lk = [X(0), X(1), X(2), X(0)], [L(0), L(0), L(1), L(3)]
    g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(50.0, 40.0, 60.0), model3, X(1), L(1), CAL_ST, stereo_sensor))
    if as_block:
        g.push_back(gtsam.ProjectionFactorBlock(uv, model2, pk, lk, CAL, mono_sensor))
    else:
        for a in range(4):
            g.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(*uv[a]), model2, pk[a], lk[a], CAL, mono_sensor))
    g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(51.0, 41.0, 61.0), model3, X(2), L(2), CAL_ST, stereo_sensor))
    return g


def _rows(pg):
    """the packed observations as a sorted list of (pose index, landmark index, mono, u, v)"""
    m = np.asarray(pg["meas"])
    return sorted((int(p), int(l), bool(f), float(r[0]), float(r[2]))
                  for p, l, f, r in zip(pg["pose_idx"], pg["lm_idx"], pg["mono"], m))


def test_graph_records_projection_factors_column_wise():
    g = _mixed_graph(False)
    assert g.size() == 6 and g.nrFactors() == 6 and len(g._mo_pk) == 4 and len(g._st_pk) == 2 and not g._other
    meas, pk, lk, model, K, mixed = g._mono_columns()
    assert meas.shape == (4, 2) and np.array_equal(meas[2], [102.0, 202.0]) and list(pk) == [X(0), X(1), X(2), X(0)]
    assert list(lk) == [L(0), L(0), L(1), L(3)] and model is MODEL2 and K is CAL and not mixed
    assert L(3) in g.keys() and X(0) in g.keys()
    pg = optimizer._pack_graph(g, _values())
    assert pg["mono"].sum() == 4 and len(pg["mono"]) == 6
    assert np.array_equal(pg["mono_K"], KM) and pg["mono_sigma"] == 7.0 and pg["sigma"] == 10.0
    rows = _rows(pg)
    assert (0, 3, True, 103.0, 203.0) in rows and (1, 1, False, 50.0, 60.0) in rows


def test_projection_factor_block_equals_the_same_factors_pushed_singly():
    a, b = optimizer._pack_graph(_mixed_graph(False), _values()), optimizer._pack_graph(_mixed_graph(True), _values())
    assert _rows(a) == _rows(b)
    for key in ("mono_K", "mono_sigma", "sigma", "loss", "body_P_sensor"):
        assert np.array_equal(a[key], b[key]), key
    assert _mixed_graph(True).nrFactors() == 6


def test_a_graph_of_mono_factors_only_packs():
    g = gtsam.NonlinearFactorGraph()
    rob = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(1.345), MODEL2)
    Sp = gtsam.Pose3.from_flat12(S)
    for i in range(3):
        g.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(1.0 + i, 2.0), rob, X(i), L(0), CAL, Sp))
    pg = optimizer._pack_graph(g, _values())
    assert pg["mono"].all() and pg["loss"] == (1, 1.345) and np.allclose(pg["body_P_sensor"], S)


def test_refusals():
    vals = _values()
    Sp = gtsam.Pose3.from_flat12(S)
    diag2 = gtsam.noiseModel.Diagonal.Sigmas(np.array([1.0, 2.0]))
    huber = lambda k, base: gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(k), base)
    cauchy = lambda k, base: gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Cauchy.Create(k), base)
    for as_block in (False, True):
        with pytest.raises(NotImplementedError, match="isotropic 2-dimensional"):
            optimizer._pack_graph(_mixed_graph(as_block, model2=diag2), vals)
        with pytest.raises(NotImplementedError, match="share one\\s+body_P_sensor|share one body_P_sensor"):
            optimizer._pack_graph(_mixed_graph(as_block, mono_sensor=Sp), vals)
        with pytest.raises(NotImplementedError, match="mEstimator"):
            optimizer._pack_graph(_mixed_graph(as_block, model2=huber(1.345, MODEL2)), vals)
        with pytest.raises(NotImplementedError, match="mEstimator"):
            optimizer._pack_graph(_mixed_graph(as_block, model2=huber(1.345, MODEL2), model3=huber(2.0, MODEL3)), vals)
        with pytest.raises(NotImplementedError, match="mEstimator"):
            optimizer._pack_graph(_mixed_graph(as_block, model2=huber(1.345, MODEL2), model3=cauchy(1.345, MODEL3)), vals)
        # the same mEstimator with different sigmas, and one extrinsic on both kinds, are accepted
        pg = optimizer._pack_graph(_mixed_graph(as_block, model2=huber(1.345, MODEL2), model3=huber(1.345, MODEL3),
                                                mono_sensor=Sp, stereo_sensor=gtsam.Pose3.from_flat12(S)), vals)
        assert pg["loss"] == (1, 1.345) and pg["sigma"] == 10.0 and pg["mono_sigma"] == 7.0
    # differing models / calibrations / extrinsics among the mono factors themselves
    for kw in (dict(model=gtsam.noiseModel.Isotropic.Sigma(2, 8.0)), dict(K=gtsam.Cal3_S2(*(KM + 1.0))), dict(sensor=Sp)):
        g = _mixed_graph(False)
        g.push_back(gtsam.GenericProjectionFactorCal3_S2(gtsam.Point2(1, 2), kw.get("model", MODEL2), X(2), L(3),
                                                         kw.get("K", CAL), kw.get("sensor")))
        with pytest.raises(NotImplementedError, match="monocular projection factors of one graph must share"):
            optimizer._pack_graph(g, vals)
        g = _mixed_graph(True)
        g.push_back(gtsam.ProjectionFactorBlock([[1.0, 2.0]], kw.get("model", MODEL2), [X(2)], [L(3)], kw.get("K", CAL),
                                                kw.get("sensor")))
        with pytest.raises(NotImplementedError, match="monocular projection factors of one graph must share"):
            optimizer._pack_graph(g, vals)


def test_problem_topology():
    import mono_problem
    seq = mono_problem.mixed_sequence()
    mono_problem.check_topology(seq)
    again = mono_problem.mixed_sequence()
    assert np.array_equal(seq["mono"], again["mono"]) and np.array_equal(seq["meas"], again["meas"], equal_nan=True)
