"""The two-point RANSAC on the front end's own temporal matches of the rendered sea-floor scene: bit-equal to its numpy
statement with the rotation from the gyro and from the odometry, the camera-to-body extrinsic conjugates that rotation,
fewer wrong matches survive than entered, and the optimised trajectory does not get worse.

Ground truth of a match: the ray of the left camera through (x1, y1), intersected with the sea-floor plane and projected
with the true poses into the next frame, lands within 4 px of (x2, y2).

Figures (6 keyframes at 1280 x 720, 2000 keypoints, track_max_distance=64, no mutual filter; profiles/ransac.md): wrong
share 48.0 % -> 1.3 % with the gyro's rotation (99.8 % of the correct matches kept), 48.0 % -> 1.2 % with the odometry's
(77.7 % kept); mean position error 1.87 mm with the parent's defaults and 1.87 mm with ransac_px=3, 71.5 mm without the
gate."""
import numpy as np
import pytest
import torch

import ransac_ref as R
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

F, H, W, KP = 6, 720, 1280, 2000
THRESHOLD = 3.0
GT_PX = 4.0


@pytest.fixture(scope="module")
def scene():
    return synth.scene_sequence(F, H, W)


@pytest.fixture(scope="module")
def front(gpu, scene):
    """The front end at track_max_distance=64 without the mutual filter, and its temporal table before any rejection."""
    from visual_underwater_slam_amd.frontend import StereoOrbFrontend, ImageProcessorParams
    prm = ImageProcessorParams(max_features=KP, track_max_distance=64, cross_check=False, ransac_threshold=THRESHOLD,
                               ransac_hypotheses=256)
    fe = StereoOrbFrontend(H, W, max_frames=F, params=prm)
    res = fe.process(torch.from_numpy(scene["frames"]).cuda())
    torch.cuda.synchronize()
    before = res.track_idx.clone()
    host = dict(track_idx=before.cpu().numpy(), kp_keys=res.kp_keys.cpu().numpy().view(np.uint32),
                kp_count=res.kp_count.cpu().numpy())
    return fe, res, before, host


def _rotations(scene, kind):
    from visual_underwater_slam_amd import sequence
    if kind == "imu":
        dR = sequence.imu_delta_rotations(scene["imu"], sequence.BatchSequence(device="cuda:0").PARAMS)
    else:
        Rb = scene["poses_init"][:, :9].reshape(-1, 3, 3)
        dR = np.einsum("pji,pjk->pik", Rb[:-1], Rb[1:])
    return sequence.ransac_rotations(dR)


def _reject(front, rot):
    fe, res, before, _ = front
    res.track_idx.copy_(before)
    info = fe.reject_track_outliers(res, torch.from_numpy(rot).cuda())
    torch.cuda.synchronize()
    out = res.track_idx.cpu().numpy().copy()
    res.track_idx.copy_(before)
    return out, info.cpu().numpy()


def correct_matches(scene, host):
    """[F-1, K] bool: the match of slot i is geometrically right (False where there is no match)."""
    fx, fy, cx, cy = synth.INTRINSIC
    sx, sy = synth.RES_X / W, synth.RES_Y / H
    trk = host["track_idx"]
    ok = np.zeros(trk.shape, bool)
    for p in range(F - 1):
        nl, nn = min(int(host["kp_count"][2 * p]), KP), min(int(host["kp_count"][2 * p + 2]), KP)
        src = np.nonzero((trk[p, :nl] >= 0) & (trk[p, :nl] < nn))[0]
        x1, y1 = R.decode(host["kp_keys"][2 * p, src], W)
        x2, y2 = R.decode(host["kp_keys"][2 * p + 2, trk[p, src]], W)
        T0, T1 = scene["poses_gt"][p], scene["poses_gt"][p + 1]
        R0, R1 = T0[:9].reshape(3, 3), T1[:9].reshape(3, 3)
        ray = np.stack([(x1 * sx - cx) / fx, (y1 * sy - cy) / fy, np.ones_like(x1)], 1) @ R0.T
        lam = (synth.SCENE_PLANE_Z - T0[11]) / ray[:, 2]
        q = (T0[9:] + ray * lam[:, None] - T1[9:]) @ R1
        u, v = (q[:, 0] / q[:, 2] * fx + cx) / sx, (q[:, 1] / q[:, 2] * fy + cy) / sy
        ok[p, src] = np.hypot(u - x2, v - y2) <= GT_PX
    return ok


@pytest.mark.parametrize("kind", ["imu", "odom"])
def test_front_end_tables_equal_the_reference(front, scene, kind):
    _, _, _, host = front
    rot = _rotations(scene, kind)
    out, info = _reject(front, rot)
    ref_out, ref_info = R.two_point_ransac(host["track_idx"], host["kp_keys"], host["kp_count"], H, W, rot,
                                           R.default_cam(H, W), THRESHOLD, 256, synth.SEED)
    assert np.array_equal(info, ref_info), (info.tolist(), ref_info.tolist())
    assert np.array_equal(out, ref_out)
    assert (info[:, 0] > 300).all() and (info[:, 2] >= 0).all()


def test_share_of_wrong_matches_drops(front, scene):
    """The share of wrong matches among the survivors is lower than in the table the matcher left (what the parent commit
    hands to vus_track_ids).  No number is fixed in advance; the figures go to profiles/ransac.md."""
    _, _, _, host = front
    ok = correct_matches(scene, host)
    had = (host["track_idx"] >= 0) & (np.arange(KP)[None, :] < np.minimum(host["kp_count"][0:2 * F - 2:2], KP)[:, None])
    for kind in ("imu", "odom"):
        out, info = _reject(front, _rotations(scene, kind))
        live = out >= 0
        wrong_before = 1.0 - ok[had].mean()
        wrong_after = 1.0 - ok[live].mean()
        kept_correct = (live & ok).sum() / ok.sum()
        print(f"ransac[{kind}]: matches {int(had.sum())} -> {int(live.sum())}; wrong share {wrong_before:.4f} -> "
              f"{wrong_after:.4f}; correct matches kept {kept_correct:.4f}; per pair {info.tolist()}")
        assert ok.sum() > 300 * (F - 1) and (had & ~ok).sum() > 0
        assert wrong_after < wrong_before


def test_body_P_sensor_conjugates_the_rotation(front, scene):
    """run_sequence with a non-identity extrinsic (the camera turned 90 degrees about the body's z axis; body poses, gyro,
    accelerometer and DVL expressed in that body frame) rejects exactly what the camera-frame rotation passed directly
    rejects."""
    from visual_underwater_slam_amd import sequence, gtsam
    fe, res, before, host = front
    Rs = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    S = gtsam.Pose3(gtsam.Rot3(Rs), np.zeros(3))
    body = np.stack([gtsam.Pose3.from_flat12(T).compose(S.inverse()).flat12() for T in scene["poses_init"]])
    imu_b = scene["imu"].copy()
    imu_b[:, :, 0:3] = scene["imu"][:, :, 0:3] @ Rs.T
    imu_b[:, :, 3:6] = scene["imu"][:, :, 3:6] @ Rs.T
    dvl_b = scene["dvl"] @ Rs.T
    direct, info_direct = _reject(front, _rotations(scene, "imu"))
    _, _, st = sequence.run_sequence(torch.from_numpy(scene["frames"]).cuda(), body, imu_b, dvl_b, disparity_sign=1,
                                     frontend=fe, body_P_sensor=S, ransac_px=THRESHOLD, ransac_rotation="imu")
    assert np.array_equal(st["frontend"].track_idx.cpu().numpy(), direct)
    assert np.array_equal(st["ransac_info"].cpu().numpy(), info_direct)
    assert not np.array_equal(direct, host["track_idx"])


def _mean_position_error(results, scene):
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    got = np.stack([results.atPose3(X(i)).flat12() for i in range(F)])
    return float(np.linalg.norm(got[:, 9:] - scene["poses_gt"][:, 9:], axis=1).mean())


def test_trajectory_is_no_worse_with_the_ransac(gpu, scene):
    """run_sequence(ransac_px=3), default gate, against run_sequence with the parent's defaults on the same scene: mean
    position error at most 1.5 x (the two runs use different factor sets).  The run without the gate is printed only."""
    from visual_underwater_slam_amd import sequence
    frames = torch.from_numpy(scene["frames"]).cuda()
    args = (frames, scene["poses_init"], scene["imu"], scene["dvl"])
    r0, _, s0 = sequence.run_sequence(*args, disparity_sign=1)
    r1, _, s1 = sequence.run_sequence(*args, disparity_sign=1, ransac_px=THRESHOLD)
    e0, e1 = _mean_position_error(r0, scene), _mean_position_error(r1, scene)
    assert "ransac_info" in s1 and "ransac_info" not in s0
    try:
        r2, _, s2 = sequence.run_sequence(*args, disparity_sign=1, ransac_px=THRESHOLD, gate_px=0)
        e2, n2 = _mean_position_error(r2, scene), int(s2["factors"]["obs_frame"].numel())
    except Exception as exc:                       # recorded, not asserted
        e2, n2 = float("nan"), repr(exc)
    print(f"mean position error: parent defaults {1e3 * e0:.2f} mm ({int(s0['factors']['obs_frame'].numel())} factors); "
          f"ransac_px=3 {1e3 * e1:.2f} mm ({int(s1['factors']['obs_frame'].numel())} factors); "
          f"ransac_px=3 gate_px=0 {1e3 * e2:.2f} mm ({n2} factors); ransac info {s1['ransac_info'].cpu().numpy().tolist()}")
    assert e1 <= 1.5 * e0, (e1, e0)
