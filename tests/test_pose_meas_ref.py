"""Position and attitude fixes on poses without a GPU: the numpy reference (tests/pose_meas_ref.py) against central
differences through the shim's Pose3.retract and against the 60-digit fixture tests/golden/pose_meas_general_position.npz,
the host-side CSR of ba.PoseMeasurements, the four shim classes and the packer."""
import os

import numpy as np
import pytest

import visual_underwater_slam_amd.gtsam as gtsam
from visual_underwater_slam_amd.gtsam import optimizer
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
import general_position
import pose_meas_ref as pmr

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pose_meas_general_position.npz")
OUTPUTS = ("Hpp", "gp", "err", "eval", "error", "weights")


def _pose(seed):
    rng = np.random.default_rng(seed)
    return gtsam.Pose3(gtsam.Rot3.Expmap(rng.uniform(-1.5, 1.5, 3)), rng.uniform(-30, 30, 3))


def test_position_jacobian_against_central_differences():
    """J = [ -R [a]x , R ] against central differences of t + R a - m through Pose3.retract (X Exp(xi)), h = 1e-5: the
    truncation is h^2 |a| / 6 ~ 2e-11 and the cancellation eps |t| / h ~ 1e-10 per entry, the bound 1e-7 is the issue's"""
    rng = np.random.default_rng(5)
    for seed in range(4):
        T = _pose(seed)
        m9 = np.concatenate([T.translation() + rng.standard_normal(3), rng.uniform(-1, 1, 3) if seed else np.zeros(3), np.zeros(3)])
        r0, J = pmr.raw_factor(pmr.POSITION, m9, T.flat12())
        h, num = 1e-5, np.zeros((3, 6))
        for c in range(6):
            e = np.zeros(6)
            e[c] = h
            rp, _ = pmr.raw_factor(pmr.POSITION, m9, T.retract(e).flat12())
            rm, _ = pmr.raw_factor(pmr.POSITION, m9, T.retract(-e).flat12())
            num[:, c] = (rp - rm) / (2 * h)
        print(f"position Jacobian vs central differences, pose {seed}: {np.abs(J - num).max():.3g}")
        assert np.abs(J - num).max() <= 1e-7
        assert np.allclose(r0, T.translation() + T.rotation().matrix() @ m9[3:6] - m9[:3], rtol=0, atol=1e-13)


def test_gp_is_the_gradient_of_the_gaussian_error_for_the_position_kind():
    """gp = sum J^T r against central differences of 0.5 sum |W r|^2 over the pose's tangent (several factors on one pose,
    per-axis sigmas, a lever arm); and the rotation kind's stated J = [I, 0] is what it says"""
    T = _pose(11)
    f12 = T.flat12()[None]
    G = pmr.PoseMeasSet([0, 0, 0], [0, 0, 0],
                        [pmr.position_meas(f12[0], [0.3, -0.5, 0.2], np.array([0.4, -0.1, 0.2])),
                         pmr.position_meas(f12[0], np.zeros(3), np.array([5.0, 3.0, -0.01])),
                         pmr.position_meas(f12[0], [-0.6, 0.1, 0.4], np.array([-0.2, 0.3, 0.1]))],
                        [[0.3, 0.2, 0.5], [1e3, 1e3, 0.02], [0.05, 0.7, 2.0]])
    H, g, e0, fac = pmr.blocks(G, f12)
    assert e0 == pytest.approx(pmr.error(G, f12), rel=1e-15)
    h, num = 1e-6, np.zeros(6)
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        num[c] = (pmr.error(G, T.retract(d).flat12()[None]) - pmr.error(G, T.retract(-d).flat12()[None])) / (2 * h)
    print(f"gp {g[0]} vs differences {num}")
    assert np.allclose(g[0], num, rtol=1e-6, atol=1e-6 * np.abs(g[0]).max())
    assert np.allclose(H[0].reshape(6, 6), H[0].reshape(6, 6).T, rtol=1e-15)
    # the linear error is the quadratic model of the blocks
    d = np.array([[0.01, -0.02, 0.005, 0.1, -0.2, 0.05]])
    assert pmr.linear_error(fac, d) == pytest.approx(e0 + float(g[0] @ d[0]) + 0.5 * float(d[0] @ H[0].reshape(6, 6) @ d[0]), rel=1e-12)
    r, J = pmr.raw_factor(pmr.ROTATION, pmr.rotation_meas(f12[0], [0.1, -0.2, 0.3]), f12[0])
    assert np.allclose(r, [0.1, -0.2, 0.3], rtol=0, atol=1e-15) and np.array_equal(J, np.hstack([np.eye(3), np.zeros((3, 3))]))
    for w in ([1e-9, 0.0, 0.0], [0.0, 2.0, 2.0], [1.8, -1.8, 1.8]):           # up to 3.118 rad
        assert np.allclose(pmr.so3_log(pmr.so3_exp(w)), w, rtol=0, atol=1e-14), w


def _fixture_set(c):
    return pmr.PoseMeasSet(c["idx"], c["kind"], c["meas"], c["sigmas"],
                           list(zip(c["loss_kind"].tolist(), c["loss_k"].reshape(-1).tolist())))


def fixture_outputs_numpy(c):
    G = _fixture_set(c)
    H, g, e, fac = pmr.blocks(G, c["poses"])
    return {"Hpp": H, "gp": g, "err": np.array([[e]]),
            "eval": np.array([[pmr.linear_error(fac, c["dp"])], [pmr.error(G, c["new_poses"])]]),
            "error": np.array([[pmr.error(G, c["poses"])]]), "weights": pmr.weights(G, c["poses"])[G.csr_order()].reshape(-1, 1)}


def test_the_fixture_holds_the_cases_it_names():
    c = dict(np.load(FIXTURE))
    G = _fixture_set(c)
    idx, kind = c["idx"], c["kind"]
    assert (idx == 3).sum() == 5 and set(kind[idx == 3].tolist()) == {0, 1} and (np.diff(idx) < 0).any()
    ang = np.array([np.linalg.norm(pmr.raw_factor(1, c["meas"][f], c["poses"][idx[f]])[0]) for f in range(G.n) if kind[f] == 1])
    assert (np.abs(ang - 1e-9) < 1e-12).any() and (np.abs(ang - (np.pi - 1e-3)) < 1e-9).any() and ((ang > 0.2) & (ang < 2.6)).any()
    assert np.abs(c["poses"][:, 9:]).max() > 900.0
    arms = np.linalg.norm(c["meas"][kind == 0, 3:6], axis=1)
    assert arms.max() > 0.5 and arms.max() <= 1.0 and (arms == 0).any()
    assert (c["sigmas"].max(1) / c["sigmas"].min(1) >= 1e5 - 1e-6).any()
    w = pmr.weights(G, c["poses"])
    d = np.array([np.sqrt(2.0 * pmr._wl(0, 0.0, float(((G.w[f] * pmr.raw_factor(int(kind[f]), G.meas[f], c["poses"][idx[f]])[0]) ** 2).sum()))[1])
                  for f in range(G.n)])
    for lk in range(1, 6):                                  # each robust loss on both sides of its threshold
        sel = c["loss_kind"] == lk
        k = c["loss_k"].reshape(-1)[sel]
        assert (d[sel] > k).any() and (d[sel] < k).any(), lk
    assert (c["loss_kind"] == 0).sum() == 4 and (w[c["loss_kind"] == 0] == 1.0).all() and (w == 0.0).any()
    for k in OUTPUTS:
        assert c["want_" + k].shape[0] == c["tol_" + k].shape[0] and "oracle_ratio_" + k in c


def test_numpy_reference_is_inside_every_bound_of_the_fixture():
    c = dict(np.load(FIXTURE))
    r = general_position.ratios(fixture_outputs_numpy(c), c, OUTPUTS)
    print({k: f"{v:.3g}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    for k, v in r.items():                                  # what the generator recorded, on its machine's libm
        assert float(c["oracle_ratio_" + k]) <= 1.0


def test_pose_meas_host_csr():
    """ba.PoseMeasurements sorts stably by pose and builds its CSR with numpy before anything is uploaded"""
    from visual_underwater_slam_amd import ba
    idx = [7, 2, 7, 0, 9, 7, 2]
    order, row_pose, row_ptr = ba.csr_rows(idx)
    assert order.tolist() == [3, 1, 6, 0, 2, 5, 4]              # graph order within one pose
    assert row_pose.tolist() == [0, 2, 7, 9] and row_ptr.tolist() == [0, 1, 3, 6, 7]
    assert row_pose.dtype == np.int32 and row_ptr.dtype == np.int32
    kind = np.array([0, 1, 0, 0, 1, 1, 0])
    meas = np.arange(63.0).reshape(7, 9)
    sig = 1.0 + np.arange(21.0).reshape(7, 3)
    losses = [None, ("huber", 1.5), (2, 0.7), None, None, ("welsch", 3.0), None]
    M = ba.PoseMeasurements(idx, kind, meas, sig, 10, pose_stride=2, loss=losses, device="cpu")
    assert (M.n, M.n_poses, M.pose_stride, M.n_rows) == (7, 10, 2, 4)
    assert (M.c.n, M.c.n_poses, M.c.pose_stride, M.c.n_rows) == (7, 10, 2, 4) and M.robust and M.addr()
    assert np.array_equal(M.host["idx"], [0, 2, 2, 7, 7, 7, 9]) and np.array_equal(M.host["meas"], meas[order])
    assert np.array_equal(M.kind.numpy(), kind[order]) and np.array_equal(M.w.numpy(), 1.0 / sig[order])
    assert M.loss_kind.tolist() == [0, 1, 0, 0, 2, 5, 0] and M.loss_k.tolist() == [0.0, 1.5, 0.0, 0.0, 0.7, 3.0, 0.0]
    assert M.row_pose.tolist() == [0, 2, 7, 9] and M.row_ptr.tolist() == [0, 1, 3, 6, 7] and np.array_equal(M.order, order)
    one = ba.PoseMeasurements(idx, kind, meas, sig, 10, loss=("cauchy", 2.0), device="cpu")
    assert one.loss_kind.tolist() == [2] * 7 and not ba.PoseMeasurements(idx, kind, meas, sig, 10, device="cpu").robust
    empty = ba.PoseMeasurements([], [], np.zeros((0, 9)), np.zeros((0, 3)), 10, device="cpu")
    assert (empty.n, empty.n_rows) == (0, 0) and empty.c.row_pose is None and empty.c.w is None and not empty.robust
    assert ba.csr_rows([])[2].tolist() == [0]
    for bad in (dict(pose_idx=[0, 10]), dict(pose_idx=[-1, 0]), dict(kind=[0, 2]), dict(meas=np.zeros((3, 9))),
                dict(sigmas=np.zeros((2, 3))), dict(sigmas=np.full((2, 3), np.inf)), dict(meas=np.full((2, 9), np.nan)),
                dict(loss=[None]), dict(pose_stride=4)):
        kw = dict(pose_idx=[0, 1], kind=[0, 1], meas=np.zeros((2, 9)), sigmas=np.ones((2, 3)), n_poses=10, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError, match="pose measurements|pose_stride"):
            ba.PoseMeasurements(**kw)
    with pytest.raises(ValueError, match="robust loss"):
        ba.PoseMeasurements([0], [0], np.zeros((1, 9)), np.ones((1, 3)), 10, loss=("nope", 1.0), device="cpu")


DIAG = gtsam.noiseModel.Diagonal.Sigmas(np.array([1e3, 1e3, 0.02]))
ISO = gtsam.noiseModel.Isotropic.Sigma(3, 0.5)
UNIT = gtsam.noiseModel.Unit.Create(3)
ROBUST = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Cauchy.Create(2.5), ISO)


def test_shim_constructors_accessors_and_refusals():
    Rm = gtsam.Rot3.Ypr(0.3, -0.2, 0.1)
    T = gtsam.Pose3(Rm, [1.0, 2.0, 3.0])
    g = gtsam.GPSFactor(X(1), gtsam.Point3(4.0, 5.0, 6.0), DIAG)
    assert g.keys() == [X(1)] and np.array_equal(g.measurementIn(), [4.0, 5.0, 6.0]) and g.noiseModel() is DIAG
    a = gtsam.GPSFactorArm(X(2), [4.0, 5.0, 6.0], [0.1, 0.2, -0.3], ROBUST)
    assert np.array_equal(a.measurementIn(), [4.0, 5.0, 6.0]) and np.array_equal(a.leverArm(), [0.1, 0.2, -0.3])
    assert a.noiseModel().robust().k == 2.5
    t1, t2 = gtsam.PoseTranslationPrior3D(X(0), T, ISO), gtsam.PoseTranslationPrior3D(X(0), np.array([1.0, 2.0, 3.0]), UNIT)
    assert np.array_equal(t1.measured(), [1.0, 2.0, 3.0]) and np.array_equal(t2.measured(), [1.0, 2.0, 3.0])
    r1, r2 = gtsam.PoseRotationPrior3D(X(0), Rm, ISO), gtsam.PoseRotationPrior3D(X(0), T, ISO)
    assert r1.measured().equals(Rm, 0.0) and r2.measured().equals(Rm, 0.0) and isinstance(r1.measured(), gtsam.Rot3)
    for name in ("GPSFactor", "GPSFactorArm", "PoseTranslationPrior3D", "PoseRotationPrior3D"):
        assert name in gtsam.__all__ and hasattr(gtsam, name)
    assert [f._kind for f in (g, a, t1, r1)] == [0, 0, 0, 1]
    assert np.array_equal(a._row9(), [4.0, 5.0, 6.0, 0.1, 0.2, -0.3, 0.0, 0.0, 0.0]) and np.array_equal(r1._row9(), Rm.matrix().reshape(9))
    six, two = gtsam.noiseModel.Isotropic.Sigma(6, 1.0), gtsam.noiseModel.Isotropic.Sigma(2, 1.0)
    for make in (lambda m: gtsam.GPSFactor(X(0), np.zeros(3), m), lambda m: gtsam.GPSFactorArm(X(0), np.zeros(3), np.zeros(3), m),
                 lambda m: gtsam.PoseTranslationPrior3D(X(0), np.zeros(3), m), lambda m: gtsam.PoseRotationPrior3D(X(0), Rm, m)):
        for m in (six, two, gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(1.0), six)):
            with pytest.raises(RuntimeError, match="3-dimensional"):
                make(m)
    for bad in (lambda: gtsam.GPSFactor(X(0), np.zeros(2), ISO), lambda: gtsam.GPSFactor(X(0), [0.0, np.nan, 0.0], ISO),
                lambda: gtsam.GPSFactorArm(X(0), np.zeros(3), np.zeros(4), ISO),
                lambda: gtsam.GPSFactorArm(X(0), np.zeros(3), [np.inf, 0.0, 0.0], ISO),
                lambda: gtsam.PoseTranslationPrior3D(X(0), np.zeros(6), ISO),
                lambda: gtsam.PoseRotationPrior3D(X(0), np.eye(3), ISO),                          # not a Rot3
                lambda: gtsam.PoseRotationPrior3D(X(0), gtsam.Rot3(1.001 * np.eye(3)), ISO),      # not orthonormal
                lambda: gtsam.PoseRotationPrior3D(X(0), gtsam.Rot3(np.diag([1.0, 1.0, -1.0])), ISO)):   # a reflection
        with pytest.raises(RuntimeError):
            bad()


def _values():
    v = gtsam.Values()
    for i in (0, 2, 5, 9):
        v.insert(X(i), gtsam.Pose3(gtsam.Rot3.Rz(0.1 * i), [1.0 * i, 0.0, -2.0]))
    v.insert(L(0), np.array([0.5, 0.0, 4.0]))
    return v


def _graph():
    g = gtsam.NonlinearFactorGraph()
    g.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3(), gtsam.noiseModel.Isotropic.Sigma(6, 0.1)))
    g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(50.0, 40.0, 60.0), gtsam.noiseModel.Isotropic.Sigma(3, 10.0), X(2), L(0),
                                            gtsam.Cal3_S2Stereo(1827.0, 1827.6, 0.0, 968.9, 561.4, 0.063)))
    return g


def test_packer_collects_all_four_classes():
    Rm = gtsam.Rot3.Ypr(0.3, -0.2, 0.1)
    g = _graph()
    assert optimizer._pack_graph(g, _values(), device=None)["pose_meas"] is None
    g.add(gtsam.PoseRotationPrior3D(X(9), Rm, gtsam.noiseModel.Diagonal.Sigmas(np.array([0.01, 0.02, 0.03]))))
    g.add(gtsam.GPSFactor(X(5), [4.0, 5.0, 6.0], DIAG))
    g.add(gtsam.GPSFactorArm(X(9), [7.0, 8.0, 9.0], [0.1, 0.2, -0.3], ROBUST))
    g.add(gtsam.PoseTranslationPrior3D(X(0), gtsam.Pose3(Rm, [1.0, 2.0, 3.0]), UNIT))
    assert g.nrFactors() == 6
    pg = optimizer._pack_graph(g, _values(), device=None)
    assert list(pg["pose_keys"]) == [X(0), X(2), X(5), X(9)]
    pm = pg["pose_meas"]
    assert pm["idx"].tolist() == [3, 2, 3, 0] and pm["kind"].tolist() == [1, 0, 0, 0]          # graph order, pose indices
    assert pm["keys"].tolist() == [X(9), X(5), X(9), X(0)]
    want = np.array([Rm.matrix().reshape(9), [4, 5, 6, 0, 0, 0, 0, 0, 0], [7, 8, 9, 0.1, 0.2, -0.3, 0, 0, 0], [1, 2, 3, 0, 0, 0, 0, 0, 0]])
    assert np.array_equal(pm["meas"], want)
    assert np.array_equal(pm["sigmas"], [[0.01, 0.02, 0.03], [1e3, 1e3, 0.02], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]])
    assert pm["losses"] == [(0, 0.0), (0, 0.0), (2, 2.5), (0, 0.0)]
    # the packed arrays are what ba.PoseMeasurements takes
    from visual_underwater_slam_amd import ba
    M = ba.PoseMeasurements(pm["idx"], pm["kind"], pm["meas"], pm["sigmas"], 4, loss=list(pm["losses"]), device="cpu")
    assert M.row_pose.tolist() == [0, 2, 3] and M.row_ptr.tolist() == [0, 1, 2, 4] and M.order.tolist() == [3, 1, 0, 2] and M.robust
    # the reference on the packed arrays: the error of the graph's four factors, stated by hand
    G = pmr.PoseMeasSet(pm["idx"], pm["kind"], pm["meas"], pm["sigmas"], pm["losses"])
    v = _values()
    e_rot = 0.5 * np.sum((gtsam.Pose3.Logmap(gtsam.Pose3(Rm.inverse().compose(v.atPose3(X(9)).rotation()), np.zeros(3)))[:3]
                          / [0.01, 0.02, 0.03]) ** 2)
    e_gps = 0.5 * np.sum(((v.atPose3(X(5)).translation() - [4.0, 5.0, 6.0]) / [1e3, 1e3, 0.02]) ** 2)
    d2 = np.sum(((v.atPose3(X(9)).transformFrom([0.1, 0.2, -0.3]) - [7.0, 8.0, 9.0]) / 0.5) ** 2)
    e_arm = 0.5 * 2.5 ** 2 * np.log1p(d2 / 2.5 ** 2)
    e_tr = 0.5 * np.sum((v.atPose3(X(0)).translation() - [1.0, 2.0, 3.0]) ** 2)
    assert pmr.error(G, pg["poses"]) == pytest.approx(e_rot + e_gps + e_arm + e_tr, rel=1e-12)


def test_a_missing_key_raises():
    g = _graph()
    g.add(gtsam.GPSFactor(X(7), [4.0, 5.0, 6.0], ISO))
    with pytest.raises(RuntimeError, match="does not exist"):
        optimizer._pack_graph(g, _values(), device=None)
    g = _graph()
    g.add(gtsam.PoseRotationPrior3D(L(0), gtsam.Rot3(), ISO))           # a key of the Values, but not a Pose3
    with pytest.raises(RuntimeError, match="does not exist"):
        optimizer._pack_graph(g, _values(), device=None)
