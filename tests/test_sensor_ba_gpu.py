"""Stereo factors with a camera-to-body extrinsic on the MI355X (include/vus_sensor.h): the `_sensor` kernels stage by
stage against the numpy reference (tests/sensor_ref.py), the identity extrinsic against today's entry points, the LM
against the reference LM, the gtsam drop-in path, the marginals, and the inertial graph the extrinsic exists for.

Inertial graph, nav_sequence(16, 400, 80), sigma = 10 px, camera at X o S_NAV (measured RMS translation error against
ground truth): the same sequence without an extrinsic on its original measurements 0.006298 m; with the extrinsic
0.005936 m; the extrinsic's measurements solved while OMITTING it 0.2714 m, with Rs transposed 0.6272 m (lever arm
|ts| = 0.229 m, not scaled)."""
import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
from conftest import same_lm_trajectory
import sensor_ref

pytestmark = pytest.mark.gpu

S = sensor_ref.extrinsic()
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
LOSSES = {"gaussian": (0, 0.0), "huber": (1, 1.345), "tukey": (3, 4.6851), "cauchy": (2, 2.3849)}


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(seq, loss, sensor, **kw):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], len(seq["poses_gt"]), len(seq["points_gt"]),
                           seq["K"], seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1],
                           prior_sigmas=seq["prior_sigmas"][None], loss=loss if loss and loss[0] else None,
                           body_P_sensor=sensor, **kw)
    return prob, StereoBASolver(prob)


def _ref(oracle, prob, seq, kind, k, sensor=S):
    pk = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in prob.pk.items()}
    return sensor_ref.SensorBA(oracle, pk, seq["K"], seq["sigma"], kind, k, sensor,
                               (np.array([0]), seq["poses_gt"][:1], seq["prior_sigmas"][None]))


def _stage_sequence(size):
    """body poses X = C o S^-1 under the sequence's camera poses, 5 % outliers, landmark 7 behind every camera"""
    seq = synth.ba_sequence(*size)
    synth.inject_outliers(seq, 0.05, (50.0, 300.0))
    seq["points_init"] = seq["points_init"].copy()
    seq["points_init"][7, 2] = -1.0
    return sensor_ref.body_sequence(seq, S)


def _check_stages(oracle, size, name):
    kind, k = LOSSES[name]
    seq = _stage_sequence(size)
    prob, sv = _problem(seq, (kind, k), S)
    assert prob.has_sensor and prob.robust == (kind != 0)
    R = _ref(oracle, prob, seq, kind, k)
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv.linearize(poses, points)
    lin = R.linearize(seq["poses_init"], seq["points_init"])
    got = {"W": sv.W, "V": sv.V, "gl": sv.gl, "Hpp": sv.Hpp, "gp": sv.gp}
    errs = {key: relerr(v.cpu().numpy(), lin[key]) for key, v in got.items()}
    print(f"sensor stages {size} {name}: {errs}")
    for key, e in errs.items():
        assert e <= 1e-11, key
    assert float(sv.scal[0]) == pytest.approx(lin["err"], rel=1e-11)
    nl_err = R.error(seq["poses_init"], seq["points_init"])
    assert sv.error(poses, points) == pytest.approx(nl_err, rel=1e-11)
    # cheirality observations (judged in the CAMERA frame) are present and have zero Jacobian rows
    perm = prob.pk["perm"].cpu().numpy().astype(np.int64)
    cheir_L = prob.pk["obs_point"].cpu().numpy() == 7
    assert cheir_L.any() and not sv.W.cpu().numpy()[cheir_L].any() and not lin["W"][cheir_L].any()
    if kind == 0:
        assert np.abs(lin["W"][~cheir_L]).max(1).min() > 0
    # one trial: GPU step (its own solve), then both outputs of eval_step against the reference at that step
    sv.schur(1e-3); sv.band_solve(); sv.backsub()
    sv.eval_step(poses, points)
    dp, dl = sv.dp.cpu().numpy(), sv.dl.cpu().numpy()
    npo, npt, lin1, new1 = R.eval_step(seq["poses_init"], seq["points_init"], dp, dl)
    assert float(sv.scal[1]) == pytest.approx(lin1, rel=1e-11)
    assert float(sv.scal[2]) == pytest.approx(new1, rel=1e-11)
    assert lin1 < lin["err"]
    assert relerr(sv.new_poses.cpu().numpy(), npo) <= 1e-12
    w = sv.stereo_weights(poses, points).cpu().numpy()
    want = np.empty_like(w)
    want[perm] = lin["w"]
    assert np.abs(w - want).max() <= 1e-11
    if kind:
        assert np.all(w[seq["obs_point"] == 7] < 1.0)
    else:
        assert np.all(w == 1.0)


@pytest.mark.parametrize("name", ("gaussian", "huber", "tukey"))
def test_sensor_stages_match_the_reference(gpu, oracle, name):
    _check_stages(oracle, (60, 900, 150), name)


def test_sensor_stages_with_more_than_256_observations_of_a_keyframe(gpu, oracle):
    """every keyframe of ba_sequence(6, 600, 320) has 320 observations: the per-pose kernel's 256-thread loop wraps
    before the congruence of its epilogue"""
    assert np.bincount(synth.ba_sequence(6, 600, 320)["obs_pose"]).min() > 256
    _check_stages(oracle, (6, 600, 320), "huber")


@pytest.mark.parametrize("name", ("gaussian", "huber"))
def test_identity_extrinsic_equals_todays_entry_points(gpu, name):
    seq = _stage_sequence((60, 900, 150))
    loss = LOSSES[name]
    prob_s, sv_s = _problem(seq, loss, IDENTITY)
    prob_0, sv_0 = _problem(seq, loss, None)
    assert prob_s.has_sensor and not prob_0.has_sensor
    poses, points = d(seq["poses_init"]), d(seq["points_init"])
    sv_s.linearize(poses, points)
    sv_0.linearize(poses, points)
    for a, b in ((sv_s.W, sv_0.W), (sv_s.V, sv_0.V), (sv_s.gl, sv_0.gl), (sv_s.Hpp, sv_0.Hpp), (sv_s.gp, sv_0.gp),
                 (sv_s.scal[:1], sv_0.scal[:1])):
        assert relerr(a.cpu().numpy(), b.cpu().numpy()) <= 1e-14
    assert sv_s.error(poses, points) == pytest.approx(sv_0.error(poses, points), rel=1e-14)
    assert relerr(sv_s.stereo_weights(poses, points).cpu().numpy(), sv_0.stereo_weights(poses, points).cpu().numpy()) <= 1e-14


def _lm_sequence():
    seq = synth.ba_sequence(12, 300, 60)
    mask = synth.inject_outliers(seq, 0.10, (50.0, 300.0), seed=11)
    assert mask.sum() >= 50
    return seq, sensor_ref.body_sequence(seq, S)


_lm_cache = {}


def _reference_lm(oracle, prob, body, name):
    """the reference LM of one loss, computed once and shared (read only)"""
    if name not in _lm_cache:
        _lm_cache[name] = _ref(oracle, prob, body, *LOSSES[name]).lm(body["poses_init"], body["points_init"])
    return _lm_cache[name]


@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_sensor_lm_walks_the_reference_lm(gpu, oracle, name):
    cam, body = _lm_sequence()
    prob, sv = _problem(body, LOSSES[name], S)
    rposes, rpoints, rrep = _reference_lm(oracle, prob, body, name)
    poses, points, rep = sv.optimize(d(body["poses_init"]), d(body["points_init"]))
    assert rrep["outer"] >= 3
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    # the camera poses X o S: the GPU's against the reference's (with 10 % outliers on 12 keyframes neither optimum is
    # nearer the sequence's camera poses than the start; the distance is printed only)
    cam_gpu = np.stack([sensor_ref.compose(x, S) for x in poses.cpu().numpy()])
    cam_ref = np.stack([sensor_ref.compose(x, S) for x in rposes])
    e = relerr(cam_gpu, cam_ref)
    rms = lambda c: float(np.sqrt(np.mean(np.sum((c[:, 9:] - cam["poses_gt"][:, 9:]) ** 2, 1))))
    print(f"sensor LM {name}: outer {rep.outer} tries {rep.tries}; camera poses vs reference {e:.2g}; "
          f"rms_t {rms(cam['poses_init']):.4g} -> {rms(cam_gpu):.4g}")
    assert e <= 1e-6          # the bound err_hist holds; measured 2.7e-12 (Gaussian), 3.8e-10 (Cauchy)


def _shim_graph(body, model, as_block):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    n_kf, nL = len(body["poses_gt"]), len(body["points_gt"])
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(body["poses_gt"][0]),
                                     gtsam.noiseModel.Diagonal.Sigmas(body["prior_sigmas"])))
    K = gtsam.Cal3_S2Stereo(*body["K"])
    Sp = gtsam.Pose3.from_flat12(S)
    for i in range(n_kf):
        values.insert(X(i), gtsam.Pose3.from_flat12(body["poses_init"][i]))
    for j in range(nL):
        values.insert(L(j), body["points_init"][j])
    if as_block:
        graph.push_back(gtsam.StereoFactorBlock(body["meas"], model, X(0) + body["obs_pose"].astype(np.int64),
                                                L(0) + body["obs_point"].astype(np.int64), K, Sp))
    else:
        for a in range(len(body["obs_pose"])):
            graph.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*body["meas"][a]), model,
                                                        X(int(body["obs_pose"][a])), L(int(body["obs_point"][a])), K, Sp))
    return graph, values


@pytest.mark.parametrize("as_block", (False, True))
def test_gtsam_drop_in_path_with_six_argument_factors(gpu, oracle, as_block):
    import visual_underwater_slam_amd.gtsam as gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    name = "cauchy"
    kind, k = LOSSES[name]
    _, body = _lm_sequence()
    noise = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Cauchy.Create(k),
                                           gtsam.noiseModel.Isotropic.Sigma(3, body["sigma"]))
    graph, initial = _shim_graph(body, noise, as_block)
    prob, sv = _problem(body, (kind, k), S)
    R = _ref(oracle, prob, body, kind, k)
    assert graph.error(initial) == pytest.approx(R.error(body["poses_init"], body["points_init"]), rel=1e-11)
    opt = gtsam.LevenbergMarquardtOptimizer(graph, initial, gtsam.LevenbergMarquardtParams())
    result = opt.optimize()
    rposes, rpoints, rrep = _reference_lm(oracle, prob, body, name)
    rep = opt.report()
    same_lm_trajectory(rep.iterations, rep.outer, rep.tries, rep.status, rep.err_hist, rrep)
    assert np.allclose(rep.lambda_hist, rrep["lambda_hist"], rtol=1e-12, atol=0)
    assert np.allclose(rep.err_hist, rrep["err_hist"], rtol=1e-6, atol=0)
    poses, points, _ = sv.optimize(d(body["poses_init"]), d(body["points_init"]))
    got = np.stack([result.atPose3(X(i)).flat12() for i in range(len(body["poses_gt"]))])
    got_pts = np.stack([result.atPoint3(L(j)) for j in range(len(body["points_gt"]))])
    assert relerr(got, poses.cpu().numpy()) < 1e-9 and relerr(got_pts, points.cpu().numpy()) < 1e-8
    # the marginals of the shim see the extrinsic too
    mg = gtsam.Marginals(graph, result)
    m = sv.marginals(poses, points)
    assert relerr(mg.marginalCovariance(X(3)), m.pose_cov[3].cpu().numpy()) < 1e-8


@pytest.mark.parametrize("name", ("gaussian", "cauchy"))
def test_sensor_marginals_against_dense_inverse(gpu, oracle, name):
    """pose covariances from solver.marginals against the dense inverse of the reference's full Hessian: 1e-9, the bound
    tests/test_marginals_gpu.py holds for the same comparison without an extrinsic"""
    seq = sensor_ref.body_sequence(synth.ba_sequence(12, 300, 60), S)
    prob, sv = _problem(seq, LOSSES[name], S)
    R = _ref(oracle, prob, seq, *LOSSES[name])
    poses, points = seq["poses_init"], seq["points_init"]
    m = sv.marginals(d(poses), d(points))
    Hinv = np.linalg.inv(R.full_hessian(poses, points))
    pc = m.pose_cov.cpu().numpy()
    for i in (0, 11):
        assert relerr(pc[i], Hinv[6 * i:6 * i + 6, 6 * i:6 * i + 6]) < 1e-9, i
    idx = np.r_[0:6, 66:72]
    assert relerr(m.joint([0, 11]), Hinv[np.ix_(idx, idx)]) < 1e-9


# -- the inertial graph ----------------------------------------------------------------------------------------------
# The camera must still see the landmarks from X o S, so the rotation here is Rot3.Ypr(0.3, -0.2, 0.1) WITHOUT the axis
# permutation of sensor_ref.extrinsic() (which would turn the down-looking rig's optical axis to the horizon and put the
# landmarks behind or beside it); 0.3 rad is still far enough from the identity that a transposed Rs fails (below).
S_NAV = sensor_ref.extrinsic(optical_axes=False)


def _project(T, p, K):
    """noiseless (uL, uR, v) of point p from the camera pose T, and its depth"""
    q = T[:9].reshape(3, 3).T @ (p - T[9:])
    return np.array([K[3] + K[0] * q[0] / q[2], K[3] + K[0] * (q[0] - K[5]) / q[2], K[4] + K[1] * q[1] / q[2]]), q[2]


def _nav_solve(oracle, seq, sensor):
    from test_nav_oracle import build_nav
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavFactors
    n_kf = len(seq["poses_gt"])
    _, N = build_nav(oracle, seq, zero_velocity_prior=False)
    prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, len(seq["points_gt"]), seq["K"],
                           seq["sigma"], prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None],
                           pose_stride=2, body_P_sensor=sensor)
    nav = NavFactors(seq["gravity"], imu=(N.imu_i, N.imu_j, N.imu_pim, N.imu_W),
                     dvl=(N.dvl_pose, N.dvl_meas, 1.0 / N.dvl_w), vprior=(N.vp_idx, N.vp_v, 1.0 / N.vp_w))
    sv = NavBASolver(prob, nav)
    out = sv.optimize(d(seq["poses_init"]), d(np.zeros_like(seq["vels_gt"])), d(np.zeros(6)), d(seq["points_init"]))
    p = out[0].cpu().numpy()
    return float(np.sqrt(np.mean(np.sum((p[:, 9:] - seq["poses_gt"][:, 9:]) ** 2, 1)))), out[4]


def test_inertial_graph_with_the_camera_off_the_body(gpu, oracle):
    """X, the IMU and the DVL as generated; the camera moved to X o S_NAV and every measurement regenerated as the
    projection through X_gt o S_NAV plus that observation's own noise.  The solve with the extrinsic is as good as the
    same sequence without one on its original measurements (within 2x: the same information seen through slightly
    different camera geometry); solving the moved camera's measurements while omitting the extrinsic is not."""
    assert np.abs(S_NAV[:9].reshape(3, 3) - S_NAV[:9].reshape(3, 3).T).max() > 0.5
    seq = synth.nav_sequence(16, 400, 80)
    moved = dict(seq)
    meas = np.empty_like(seq["meas"])
    for a in range(len(meas)):
        X, p = seq["poses_gt"][seq["obs_pose"][a]], seq["points_gt"][seq["obs_point"][a]]
        old, z0 = _project(X, p, seq["K"])
        new, z1 = _project(sensor_ref.compose(X, S_NAV), p, seq["K"])
        assert z0 > 0 and z1 > 0.2
        meas[a] = new + (seq["meas"][a] - old)
    moved["meas"] = meas
    base, rep0 = _nav_solve(oracle, seq, None)
    with_s, rep1 = _nav_solve(oracle, moved, S_NAV)
    omitted, _ = _nav_solve(oracle, moved, None)
    transposed, _ = _nav_solve(oracle, moved, np.concatenate([S_NAV[:9].reshape(3, 3).T.reshape(9), S_NAV[9:]]))
    print(f"inertial graph rms_t: no extrinsic {base:.4g} m, with {with_s:.4g} m, omitted {omitted:.4g} m, "
          f"transposed Rs {transposed:.4g} m; tries {rep0.tries} / {rep1.tries}")
    assert rep1.status == 0
    assert with_s <= 2.0 * base
    assert omitted > 2.0 * base and transposed > 2.0 * base


def test_sharded_solver_refuses_a_problem_with_a_sensor(gpu):
    from visual_underwater_slam_amd import dist as vdist
    seq = synth.ba_sequence(6, 40, 20)
    with pytest.raises(NotImplementedError, match="body_P_sensor"):
        vdist.ShardedStereoBASolver(seq["obs_pose"], seq["obs_point"], seq["meas"], 6, len(seq["points_gt"]), seq["K"],
                                    seq["sigma"], body_P_sensor=S)
    prob, _ = _problem(sensor_ref.body_sequence(seq, S), None, S)
    with pytest.raises(NotImplementedError, match="body_P_sensor"):
        vdist._ShardSolver(prob, 1)
