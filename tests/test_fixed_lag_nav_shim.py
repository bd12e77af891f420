"""The gtsam / gtsam_unstable side of inertial fixed-lag smoothing without a GPU: the second shape of LinearContainerFactor
(X, V, B keys) and its refusals, the forced per-keyframe layout, the timestamp rule, the layout refusals of the smoother and
the absorbed-set bookkeeping of an inertial window on keys alone."""
import numpy as np
import pytest

from visual_underwater_slam_amd import gtsam, gtsam_unstable
from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L, V, B


def _spd(rng, n):
    M = rng.normal(size=(n, n))
    return M @ M.T + n * np.eye(n)


def _values(n=5):
    v = gtsam.Values()
    for i in range(n):                               # keyframes 0, 2, 4, ..: gaps in the index
        v.insert(X(2 * i), gtsam.Pose3(gtsam.Rot3.Rz(0.1 * i), [float(i), 0.0, 0.0]))
        v.insert(V(2 * i), np.array([0.1 * i, 0.2, -0.3]))
        v.insert(B(2 * i), gtsam.imuBias.ConstantBias(np.array([0.01 * i, 0.0, 0.02]), np.array([0.0, 0.001 * i, 0.0])))
    return v


DIM = {"x": 6, "v": 3, "b": 6}


def _container(keys, values, rng, dims=None):
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import symbolChr
    dims = [DIM[symbolChr(k)] for k in keys] if dims is None else dims
    off = np.r_[0, np.cumsum(dims)]
    G = _spd(rng, off[-1])
    blocks = [G[off[a]:off[a + 1], off[b]:off[b + 1]] for a in range(len(keys)) for b in range(a, len(keys))]
    hf = gtsam.HessianFactor(keys, blocks, [rng.normal(size=d) for d in dims], 1.0)
    return hf, gtsam.LinearContainerFactor(hf, values)


def _imu(i, j, bias_key):
    params = gtsam.PreintegrationParams.MakeSharedU(9.81)
    pim = gtsam.PreintegratedImuMeasurements(params, gtsam.imuBias.ConstantBias())
    pim.integrateMeasurement(np.array([0.0, 0.0, 9.81]), np.zeros(3), 0.1)
    return gtsam.ImuFactor(X(i), V(i), X(j), V(j), bias_key, pim)


def _graph(*factors, values):
    g = gtsam.NonlinearFactorGraph()
    g.add(gtsam.PriorFactorPose3(X(0), values.atPose3(X(0)), gtsam.noiseModel.Isotropic.Sigma(6, 0.1)))
    for f in factors:
        g.add(f)
    return g


def test_the_inertial_container_is_lowered_to_a_nav_window_prior():
    rng = np.random.default_rng(1)
    v = _values()
    keys = [B(4), X(2), V(4), X(4), B(2), V(2)]              # any order; keyframes 2 and 4 are consecutive in the pose table
    hf, lc = _container(keys, v, rng)
    assert lc._is_inertial() and lc.linearizationPoint().size() == 6
    pg = _pack_graph(_graph(lc, values=v), v)
    w = pg["nav_window_prior"]
    assert pg["window_prior"] is None and w["first"] == 1 and w["c"] == 0.5
    assert w["x0"].shape == (2, 12) and np.array_equal(w["x0"], v.pose3_block([X(2), X(4)]))
    assert np.array_equal(w["v0"], np.stack([v.atVector(V(2)), v.atVector(V(4))]))
    assert np.array_equal(w["b0"], np.stack([v.atConstantBias(B(2)).vector(), v.atConstantBias(B(4)).vector()]))
    # the factor's rows: B4 0:6, X2 6:12, V4 12:15, X4 15:21, B2 21:27, V2 27:30 -> X2 V2 B2 X4 V4 B4
    perm = np.r_[6:12, 27:30, 21:27, 15:21, 12:15, 0:6]
    assert np.array_equal(w["H"], hf.information()[np.ix_(perm, perm)]) and np.array_equal(w["g"], -hf.linearTerm()[perm])
    # the container alone makes the graph an inertial one in the per-keyframe layout
    nav = pg["nav"]
    assert nav["per_keyframe"] and nav["bias_keys"] == [B(2 * i) for i in range(5)] and nav["bias"].shape == (5, 6)
    # a pose-only container still lowers to the pose-only prior
    hp = gtsam.HessianFactor([X(2)], [np.eye(6)], [np.zeros(6)], 0.0)
    lp = gtsam.LinearContainerFactor(hp, v)
    assert not lp._is_inertial()
    vp = gtsam.Values()
    for i in range(5):
        vp.insert(X(2 * i), v.atPose3(X(2 * i)))
    pg = _pack_graph(_graph(lp, values=vp), vp)
    assert pg["nav_window_prior"] is None and pg["window_prior"]["first"] == 1 and pg["nav"] is None


def test_the_container_forces_the_per_keyframe_layout():
    """A graph with one ImuFactor and no bias factor reads as the shared-bias layout; with the container, or when the caller
    asks, as one bias per keyframe."""
    rng = np.random.default_rng(2)
    v = _values(2)
    imu = _imu(0, 2, B(0))
    assert not _pack_graph(_graph(imu, values=v), v)["nav"]["per_keyframe"]
    assert _pack_graph(_graph(imu, values=v), v, None, True)["nav"]["per_keyframe"]
    lc = _container([X(2), V(2), B(2)], v, rng)[1]
    pg = _pack_graph(_graph(imu, lc, values=v), v)
    assert pg["nav"]["per_keyframe"] and pg["nav_window_prior"]["first"] == 1 and pg["nav"]["bias"].shape == (2, 6)
    # a pose-only container next to inertial factors stays refused
    hp = gtsam.HessianFactor([X(2)], [np.eye(6)], [np.zeros(6)], 0.0)
    with pytest.raises(NotImplementedError, match="LinearContainerFactor over Pose3 keys next to inertial factors"):
        _pack_graph(_graph(imu, gtsam.LinearContainerFactor(hp, v), values=v), v)


def test_inertial_container_refusals():
    rng = np.random.default_rng(3)
    v = _values()

    def pack(lc, values=v):
        return _pack_graph(_graph(lc, values=values), values)
    with pytest.raises(NotImplementedError, match=r"keyframe 4 has x4, b4 but not v4"):
        pack(_container([X(2), V(2), B(2), X(4), B(4)], v, rng)[1])
    with pytest.raises(NotImplementedError, match=r"keyframe 2 has x2, v2 but not b2"):
        pack(_container([X(2), V(2)], v, rng)[1])
    with pytest.raises(NotImplementedError, match=r"keyframe 4 has v4 but not x4, b4"):
        pack(_container([X(2), V(2), B(2), V(4)], v, rng)[1])
    with pytest.raises(NotImplementedError, match=r"key v2 has a block of 6 values, 3 are expected"):
        pack(_container([X(2), V(2), B(2)], v, rng, dims=[6, 6, 6])[1])
    with pytest.raises(NotImplementedError, match=r"key b2 has a block of 3 values, 6 are expected"):
        pack(_container([X(2), V(2), B(2)], v, rng, dims=[6, 3, 3])[1])
    with pytest.raises(NotImplementedError, match=r"x2, x6 are not consecutive"):
        pack(_container([X(2), V(2), B(2), X(6), V(6), B(6)], v, rng)[1])
    odd = _values()
    odd.erase(V(2))
    odd.insert(V(2), np.arange(4.0))
    with pytest.raises(NotImplementedError, match=r"key v2 is not a 3-vector"):
        pack(_container([X(2), V(2), B(2)], odd, rng)[1], values=odd)
    with pytest.raises(NotImplementedError, match="more than one LinearContainerFactor"):
        _pack_graph(_graph(_container([X(2), V(2), B(2)], v, rng)[1], _container([X(4), V(4), B(4)], v, rng)[1], values=v), v)
    lc = _container([X(8), V(8), B(8)], v, rng)[1]
    with pytest.raises(RuntimeError, match=r"x8.*does not exist in the Values"):
        pack(lc, values=_values(4))
    # keys that are neither shape keep the pose-only refusals
    with pytest.raises(NotImplementedError, match="not a Pose3"):
        v6 = _values()
        v6.erase(V(0))
        v6.insert(V(0), np.arange(6.0))
        pack(_container([V(0)], v6, rng, dims=[6])[1], values=v6)
    with pytest.raises(NotImplementedError, match="must be a Pose3"):
        vl = _values()
        vl.insert(L(0), np.array([1.0, 2.0, 3.0]))
        pack(_container([X(2), L(0)], vl, rng, dims=[6, 3])[1], values=vl)


def _keyframe(theta, stamps, i, t=None):
    theta.insert(X(i), gtsam.Pose3())
    theta.insert(V(i), np.zeros(3))
    theta.insert(B(i), gtsam.imuBias.ConstantBias())
    for k in (X(i), V(i), B(i)):
        stamps[k] = float(i if t is None else t)


def test_the_timestamp_rule_names_the_key():
    for bad in (V(1), B(0)):
        s = gtsam_unstable.BatchFixedLagSmoother(4.0)
        theta, stamps = gtsam.Values(), {}
        _keyframe(theta, stamps, 0)
        _keyframe(theta, stamps, 1)
        stamps[bad] += 0.5
        g = gtsam.NonlinearFactorGraph()
        g.add(_imu(0, 1, B(0)))
        name = ("v1" if bad == V(1) else "b0")
        with pytest.raises(ValueError, match=f"the key {name} has the timestamp"):
            s.update(g, theta, stamps)
        assert s.calculateEstimate().size() == 0
    # a missing timestamp keeps its own message
    s = gtsam_unstable.BatchFixedLagSmoother(4.0)
    theta, stamps = gtsam.Values(), {}
    _keyframe(theta, stamps, 0)
    _keyframe(theta, stamps, 1)
    del stamps[B(1)]
    g = gtsam.NonlinearFactorGraph()
    g.add(_imu(0, 1, B(0)))
    with pytest.raises(ValueError, match="no timestamp for the key b1"):
        s.update(g, theta, stamps)


def test_the_smoother_refuses_other_inertial_layouts_by_name():
    noise3, noise6 = gtsam.noiseModel.Isotropic.Sigma(3, 0.1), gtsam.noiseModel.Isotropic.Sigma(6, 0.1)
    bias = gtsam.imuBias.ConstantBias()
    # a keyframe without one of its three keys, before the missing-key check
    for drop, f, name in ((B(0), gtsam.DvlVelocityFactor(noise3, V(0), X(0), [0.1, 0.0, 0.0]), "DvlVelocityFactor"),
                          (V(1), gtsam.BetweenFactorConstantBias(B(0), B(1), bias, noise6), "BetweenFactorConstantBias"),
                          (X(0), gtsam.PriorFactorConstantBias(B(0), bias, noise6), "PriorFactorConstantBias"),
                          (B(1), _imu(0, 1, B(0)), "ImuFactor"),
                          (B(0), gtsam.PriorFactorVector(V(0), np.zeros(3), noise3), "PriorFactorVector")):
        s = gtsam_unstable.BatchFixedLagSmoother(4.0)
        theta, stamps = gtsam.Values(), {}
        _keyframe(theta, stamps, 0)
        _keyframe(theta, stamps, 1)
        theta.erase(drop)
        g = gtsam.NonlinearFactorGraph()
        g.add(f)
        with pytest.raises(NotImplementedError, match=name + ".*inertial") as e:
            s.update(g, theta, stamps)
        assert gtsam.symbol_shorthand.key_string(drop) in str(e.value)
    # the shared-bias layout
    s = gtsam_unstable.BatchFixedLagSmoother(4.0)
    theta, stamps = gtsam.Values(), {}
    for i in range(3):
        _keyframe(theta, stamps, i)
    g = gtsam.NonlinearFactorGraph()
    g.add(_imu(0, 1, B(0)))
    g.add(_imu(1, 2, B(0)))
    with pytest.raises(NotImplementedError, match=r"ImuFactor\(x1, .., x2\) uses the bias b0.*shared-bias.*inertial"):
        s.update(g, theta, stamps)
    g = gtsam.NonlinearFactorGraph()
    g.add(gtsam.CustomFactor(noise3, [V(0), X(0)], lambda *a: np.zeros(3)))
    with pytest.raises(NotImplementedError, match="CustomFactor.*inertial"):
        s.update(g, theta, stamps)


def test_the_absorbed_set_of_an_inertial_window_on_keys_alone():
    """Keyframes 0, 1 expired (cut = 2): their X, V and B are the expired keys.  Every inertial-side factor touching one of
    them is absorbed -- the ImuFactor 1 -> 2 and the bias walk 1 -> 2 reach into keyframe 2 -- the landmark rules are those
    of the pose-only window."""
    kf = gtsam_unstable.keyframe_keys
    assert kf(X(3)) == [X(3), V(3), B(3)]
    expired = [k for p in (X(0), X(1)) for k in kf(p)]
    ts = {**{k: float(i) for i in range(4) for k in kf(X(i))}, L(10): 0.0, L(11): 2.5}
    side = [[X(0)],                                  # pose prior
            [V(0)], [B(0)],                          # velocity and bias priors
            [X(0), V(0), X(1), V(1), B(0)],          # ImuFactor 0 -> 1
            [X(1), V(1), X(2), V(2), B(1)],          # ImuFactor 1 -> 2
            [X(2), V(2), X(3), V(3), B(2)],          # ImuFactor 2 -> 3
            [B(0), B(1)], [B(1), B(2)], [B(2), B(3)],
            [V(1), X(1)], [V(2), X(2)],              # DVL
            [V(2)]]                                  # a velocity prior on a kept keyframe
    proj = [(X(0), L(10)), (X(3), L(10)), (X(1), L(11)), (X(2), L(11))]
    a_side, a_proj, d_proj, a_pp, gone = gtsam_unstable.absorbed_set(side, proj, [L(10)], expired, ts, 2.0)
    assert a_side == [True, True, True, True, True, False, True, True, False, True, False, False]
    assert a_proj == [True, True, False, False] and d_proj == [False, False, True, False] and a_pp == [True] and gone == [L(10)]
    # the last keyframe an absorbed factor touches, through any of its three keys
    touched = {gtsam_unstable._pose_key_of(k) for keys, a in zip(side, a_side) if a for k in keys}
    assert touched == {X(0), X(1), X(2)}
    # a bias-only or velocity-only key expires with its keyframe: B(1) alone absorbs the walk 1 -> 2
    a_side, *_ = gtsam_unstable.absorbed_set([[B(1), B(2)], [B(2), B(3)]], [], [], expired, ts, 2.0)
    assert a_side == [True, False]
