"""Stereo factors with a camera-to-body extrinsic, the parts that need no GPU: the numpy reference (tests/sensor_ref.py)
against finite differences and against the plain reference at the camera pose, the gtsam shim's sixth argument, and the
host-side validation of the `_sensor` entry points (include/vus_sensor.h)."""
import ctypes

import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth, ba_pack
import robust_ref
import sensor_ref

S = sensor_ref.extrinsic()


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _small(oracle, kind=0, k=0.0, S=S, cls=sensor_ref.SensorBA):
    """ba_sequence(6, 40, 20) with body poses, one landmark behind its cameras, packed on the CPU; no priors"""
    seq = synth.ba_sequence(6, 40, 20)
    seq["points_init"] = seq["points_init"].copy()
    seq["points_init"][7, 2] = -1.0
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]),
                                   torch.from_numpy(seq["meas"]), 6, len(seq["points_gt"]))
    if cls is sensor_ref.SensorBA:
        return seq, cls(oracle, pk, seq["K"], seq["sigma"], kind, k, S)
    return seq, cls(oracle, pk, seq["K"], seq["sigma"], kind, k)


def test_extrinsic_is_a_rotation_far_from_identity():
    R = S[:9].reshape(3, 3)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and np.linalg.det(R) == pytest.approx(1.0, abs=1e-15)
    assert np.abs(R - R.T).max() > 0.5 and np.abs(R - np.eye(3)).max() > 0.9
    assert np.array_equal(S[9:], [0.05, -0.10, 0.20])
    assert relerr(sensor_ref.compose(sensor_ref.compose(np.arange(12.0), S), sensor_ref.inverse(S)), np.arange(12.0)) < 1e-14


def test_jacobians_match_central_differences(oracle):
    """H1 in the BODY tangent against central differences of the residual through the retraction of the body pose
    (step 1e-6), and H2 against differences in the point, on 20 seeded observations: 1e-6 relative."""
    seq, R = _small(oracle)
    body = sensor_ref.body_sequence(seq, S)
    poses, points = body["poses_init"], seq["points_init"]
    _, H1, H2 = R.factors(poses, points)
    rng = np.random.default_rng(3)
    front = np.nonzero(np.abs(H1).reshape(R.nO, -1).max(1) > 0)[0]         # cheirality observations have no Jacobian
    assert len(front) < R.nO
    h = 1e-6

    def resid(a, X, p):
        return oracle.stereo_factor(sensor_ref.compose(X, S), p, R.meas[a], R.K, R.w_sig)[0]
    for a in rng.choice(front, 20, replace=False):
        X, p = poses[R.op[a]], points[R.ol[a]]
        fd1 = np.zeros((3, 6)); fd2 = np.zeros((3, 3))
        for c in range(6):
            e = np.zeros(6); e[c] = h
            fd1[:, c] = (resid(a, oracle.pose_retract(X, e), p) - resid(a, oracle.pose_retract(X, -e), p)) / (2 * h)
        for c in range(3):
            e = np.zeros(3); e[c] = h
            fd2[:, c] = (resid(a, X, p + e) - resid(a, X, p - e)) / (2 * h)
        assert relerr(H1[a], fd1) <= 1e-6 and relerr(H2[a], fd2) <= 1e-6, a


@pytest.mark.parametrize("kind,k", ((0, 0.0), (2, 2.3849)))
def test_error_at_body_poses_equals_the_plain_error_at_camera_poses(oracle, kind, k):
    """Composition rounding moves a residual by ~1e-11 px against residuals of ~1 px: 1e-9 relative."""
    seq, R = _small(oracle, kind, k)
    _, P = _small(oracle, kind, k, cls=robust_ref.RobustBA)
    body = sensor_ref.body_sequence(seq, S)
    for key in ("poses_init", "poses_gt"):
        assert R.error(body[key], seq["points_init"]) == pytest.approx(P.error(seq[key], seq["points_init"]), rel=1e-9)
    r_b, _, H2_b = R.factors(body["poses_init"], seq["points_init"])
    r_c, _, H2_c = P.factors(seq["poses_init"], seq["points_init"])
    assert relerr(r_b, r_c) <= 1e-9 and relerr(H2_b, H2_c) <= 1e-9
    assert relerr(R.weights(body["poses_init"], seq["points_init"]), P.weights(seq["poses_init"], seq["points_init"])) <= 1e-9


def test_identity_extrinsic_reproduces_the_plain_reference(oracle):
    I = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    seq, R = _small(oracle, 1, 1.345, S=I)
    _, P = _small(oracle, 1, 1.345, cls=robust_ref.RobustBA)
    a, b = R.linearize(seq["poses_init"], seq["points_init"]), P.linearize(seq["poses_init"], seq["points_init"])
    for key in ("W", "V", "gl", "Hpp", "gp", "w"):
        assert relerr(a[key], b[key]) <= 1e-14, key
    assert a["err"] == pytest.approx(b["err"], rel=1e-14)
    assert R.error(seq["poses_init"], seq["points_init"]) == pytest.approx(P.error(seq["poses_init"], seq["points_init"]), rel=1e-14)


# -- the gtsam shim ---------------------------------------------------------------------------------------------------
def _shim():
    import visual_underwater_slam_amd.gtsam as gtsam
    noise = gtsam.noiseModel.Isotropic.Sigma(3, 10.0)
    K = gtsam.Cal3_S2Stereo(500.0, 500.0, 0.0, 320.0, 240.0, 0.1)
    return gtsam, noise, K, gtsam.Pose3.from_flat12(S)


def test_sixth_argument_is_stored_and_returned_as_a_copy():
    gtsam, noise, K, Sp = _shim()
    f = gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(1, 2, 3), noise, 1, 2, K, Sp)
    got = f.body_P_sensor()
    assert got is not Sp and got.equals(Sp, 1e-15)
    got._t[0] = 9.0                                             # the accessor hands out a copy
    Sp._t[1] = 9.0                                              # and the factor keeps its own
    assert np.array_equal(f.body_P_sensor().flat12(), S)
    assert gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(1, 2, 3), noise, 1, 2, K).body_P_sensor() is None
    b = gtsam.StereoFactorBlock(np.zeros((2, 3)), noise, [1, 1], [2, 3], K, gtsam.Pose3.from_flat12(S))
    assert np.array_equal(b.body_P_sensor().flat12(), S)
    assert gtsam.StereoFactorBlock(np.zeros((2, 3)), noise, [1, 1], [2, 3], K).body_P_sensor() is None
    with pytest.raises(RuntimeError, match="body_P_sensor"):
        gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(1, 2, 3), noise, 1, 2, K, S)


def _graph(factors):
    gtsam, noise, K, Sp = _shim()
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
    g, v = gtsam.NonlinearFactorGraph(), gtsam.Values()
    v.insert(X(0), gtsam.Pose3())
    for j in range(3):
        v.insert(L(j), np.array([0.1 * j, 0.0, 2.0]))
    for kind, j, sensor in factors:
        if kind == "object":
            g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(300, 280, 240), noise, X(0), L(j), K, sensor))
        else:
            g.push_back(gtsam.StereoFactorBlock(np.array([[300.0, 280, 240]]), noise, [X(0)], [L(j)], K, sensor))
    return _pack_graph(g, v, None)


def test_pack_collects_one_extrinsic_and_refuses_a_mix():
    gtsam, _, _, Sp = _shim()
    other = gtsam.Pose3.from_flat12(S + np.concatenate([np.zeros(9), [1e-9, 0, 0]]))
    near = gtsam.Pose3.from_flat12(S + np.concatenate([np.zeros(9), [1e-14, 0, 0]]))
    assert _graph([("object", 0, None), ("block", 1, None)])["body_P_sensor"] is None
    for kinds in (("object", "object"), ("object", "block"), ("block", "block")):
        pg = _graph([(kinds[0], 0, Sp), (kinds[1], 1, near)])            # equal within Pose3.equals(tol 1e-12)
        assert np.abs(pg["body_P_sensor"] - S).max() <= 1e-12             # whichever of the two was met first
        for a, b in ((Sp, None), (None, Sp), (Sp, other)):
            with pytest.raises(NotImplementedError, match="must share one"):
                _graph([(kinds[0], 0, a), (kinds[1], 1, b)])


# -- the C ABI ---------------------------------------------------------------------------------------------------------
NAMES = ("vus_ba_linearize_sensor", "vus_ba_eval_step_sensor", "vus_ba_error_sensor", "vus_ba_stereo_weights_sensor")


def test_library_exports_and_binds_the_sensor_entry_points():
    import os
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vus_sensor.h")).read()
    assert '#include "vus_sensor.h"' in open(os.path.join(root, "include", "vus.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in header
    # the plain arguments, then loss and sensor
    assert len(L.SIGNATURES["vus_ba_linearize_sensor"]) == len(L.SIGNATURES["vus_ba_linearize"]) + 2
    assert len(L.SIGNATURES["vus_ba_eval_step_sensor"]) == len(L.SIGNATURES["vus_ba_eval_step"]) + 2
    assert len(L.SIGNATURES["vus_ba_error_sensor"]) == len(L.SIGNATURES["vus_ba_error"]) + 2
    assert len(L.SIGNATURES["vus_ba_stereo_weights_sensor"]) == len(L.SIGNATURES["vus_ba_stereo_weights"]) + 1


def test_invalid_sensor_is_rejected_without_a_gpu():
    """Validation happens on the host before any launch: no device is touched, every other pointer is a dummy."""
    import visual_underwater_slam_amd._lib as L
    from visual_underwater_slam_amd.ba import _CSensor, _CLoss
    lib = L.load()

    def sensor(T):
        return _CSensor((ctypes.c_double * 12)(*T))
    nan = S.copy(); nan[10] = np.nan
    inf = S.copy(); inf[4] = np.inf
    skewed = S.copy(); skewed[0] += 1e-6
    mirror = S.copy(); mirror[:3] = -mirror[:3]
    cases = ((None, b"sensor is null"), (sensor(nan), b"not finite"), (sensor(inf), b"not finite"),
             (sensor(skewed), b"not orthonormal"), (sensor(mirror), b"reflection"))
    d8 = ctypes.c_void_p(8)
    for s, text in cases:
        sp = None if s is None else ctypes.addressof(s)
        calls = ((lib.vus_ba_linearize_sensor, (d8,) * 10 + (None, None, sp)),
                 (lib.vus_ba_eval_step_sensor, (d8,) * 9 + (None, None, sp)),
                 (lib.vus_ba_error_sensor, (d8,) * 5 + (None, None, sp)),
                 (lib.vus_ba_stereo_weights_sensor, (d8, None, d8, d8, d8, None, sp)))
        for fn, args in calls:
            assert fn(*args) == -1 and text in lib.vus_last_error(), (fn.__name__, text, lib.vus_last_error())
    # a bad loss is refused in the same place; a valid sensor with a null problem gets as far as the problem check
    bad = _CLoss(7, 1.0)
    ok = sensor(S)
    assert lib.vus_ba_error_sensor(d8, d8, d8, d8, d8, None, ctypes.addressof(bad), ctypes.addressof(ok)) == -1
    assert b"loss kind" in lib.vus_last_error()
    assert lib.vus_ba_error_sensor(None, d8, d8, d8, d8, None, None, ctypes.addressof(ok)) == -1
    assert b"problem is null" in lib.vus_last_error()


def test_problem_argument_forms():
    """sensor_flat12: a 12-vector, a 4 x 4 matrix and a Pose3 name the same extrinsic; anything else is refused."""
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.ba import sensor_flat12
    M = np.eye(4); M[:3, :3] = S[:9].reshape(3, 3); M[:3, 3] = S[9:]
    assert sensor_flat12(None) is None
    for form in (S, list(S), M, torch.from_numpy(M), gtsam.Pose3.from_flat12(S)):
        assert np.array_equal(sensor_flat12(form), S)
    with pytest.raises(ValueError):
        sensor_flat12(np.zeros((3, 4)))
    M[3, 0] = 1.0
    with pytest.raises(ValueError):
        sensor_flat12(M)


def test_sharded_solver_refuses_a_sensor():
    from visual_underwater_slam_amd import dist as vdist
    seq = synth.ba_sequence(6, 40, 20)
    with pytest.raises(NotImplementedError, match="body_P_sensor"):
        vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, len(seq["points_gt"]), seq["K"],
                                    seq["sigma"], body_P_sensor=S)
