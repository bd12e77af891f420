"""The closed survey track of the loop-closure tests: ten down-looking stereo keyframes 2 m above the textured sea floor of
synth.render_plane_view (19 px of disparity at 640 x 360), out along x, one lane over, and back, so that the last keyframe
sees the first one's ground again, turned by 25 degrees; the keyframe at the far end shares no ground with the first.
Test infrastructure only (a plain module, not a conftest): used by tests/test_loop_sequence_gpu.py and by
tools/loop_reference_error.py, which measures on the CPU what the GPU test is held to."""
import numpy as np

import loop_ref as L
from visual_underwater_slam_amd import synth

H, W, KP = 360, 640, 2000
ALTITUDE = 2.0
STEP, LANE = 0.6, 0.3
YAW_END = np.deg2rad(25.0)
N_KF = 10
REVISIT, FALSE_PAIR = (0, 9), (0, 4)        # keyframe 4 is 2.4 m out: its 2.1 m wide footprint ends 1.2 m short of keyframe 0's
THRESHOLD, N_HYP, REFINE, MATCH_DISTANCE = 2.0, 256, 10, 50
CAM5 = L.default_cam5(H, W)


def poses_gt():
    """[N_KF, 12] camera-to-world, camera z pointing down, yaw growing evenly to YAW_END."""
    xy = [(k * STEP, 0.0) for k in range(5)] + [(4 * STEP - k * STEP, LANE) for k in range(4)] + [(0.05, LANE)]
    out = []
    for k, (x, y) in enumerate(xy):
        R = L.rodrigues((0.0, 0.0, YAW_END * k / (N_KF - 1))) @ np.diag([1.0, -1.0, -1.0])
        out.append(np.concatenate([R.reshape(-1), [x, y, synth.SCENE_PLANE_Z + ALTITUDE]]))
    return np.array(out)


def poses_drifted(gt):
    """The odometry's estimate: an error that grows along the track, 2 cm and 4 mrad of yaw per keyframe (18 cm and 36 mrad
    at the last one)."""
    out = []
    for k, T in enumerate(gt):
        R = L.rodrigues((0.0, 0.0, 0.004 * k)) @ T[:9].reshape(3, 3)
        out.append(np.concatenate([R.reshape(-1), T[9:] + np.array([0.016, -0.012, 0.002]) * k]))
    return np.array(out)


def relative(gt, a, b):
    """flat12 of T_a^-1 T_b."""
    Ra, Rb = gt[a, :9].reshape(3, 3), gt[b, :9].reshape(3, 3)
    return np.concatenate([(Ra.T @ Rb).reshape(-1), Ra.T @ (gt[b, 9:] - gt[a, 9:])])


def tables(match_idx, pair_a, pair_b, stereo_idx, kp_keys, kp_count):
    """The table dict of loop_ref.stereo_pair_pose from a front end's output (host arrays)."""
    return dict(match_idx=np.asarray(match_idx, np.int32), pair_a=np.asarray(pair_a, np.int32), pair_b=np.asarray(pair_b, np.int32),
                stereo_idx=np.asarray(stereo_idx, np.int32), kp_keys=np.asarray(kp_keys).view(np.uint32),
                kp_count=np.asarray(kp_count, np.int32), H=H, W=W, cam=CAM5)
