"""What the sub-pixel tests and tools/subpixel_reference_error.py measure on the closed track of tests/loop_scene.py: the
error of a stereo disparity against the rendered geometry, and the track raised to another altitude.  Test infrastructure
only (a plain module, not a conftest)."""
import numpy as np

import loop_scene as LS
import subpixel_ref as S
from visual_underwater_slam_amd import synth

HALF_WIN, SEARCH = 5, 5                   # SubpixelParams' defaults
YAWED = range(1, LS.N_KF)                 # keyframe 0 has no yaw: its texture edges fall on whole columns in both images
NEAR_PX = 1.5                             # two independently detected corners of one point differ by a pixel or so, not more
HIGH_ALTITUDE = 4.0                       # 9.6 px of disparity at 640 x 360, where DESIGN 7l's integer bias is largest


def poses_at(altitude):
    """loop_scene.poses_gt() with the camera `altitude` metres above the sea floor."""
    gt = LS.poses_gt().copy()
    gt[:, 11] = synth.SCENE_PLANE_Z + altitude
    return gt


def true_disparity(T12, xl, yl, H=LS.H, W=LS.W):
    """fx b / Z of the sea-floor point that left pixel (xl, yl) of the camera at T12 sees, in pixels of the H x W image:
    the ray of synth.render_plane_view, whose camera-frame z component is 1, so Z is its parameter at the plane."""
    fx, fy, cx, cy = synth.INTRINSIC
    xn = (np.asarray(xl, np.float64) * (synth.RES_X / W) - cx) / fx
    yn = (np.asarray(yl, np.float64) * (synth.RES_Y / H) - cy) / fy
    Z = (synth.SCENE_PLANE_Z - T12[11]) / ((xn * T12[6] + yn * T12[7]) + T12[8])
    return (fx * W / synth.RES_X) * synth.BASELINE_M / Z


def disparity_errors(gt, stereo_idx, kp_keys, kp_count, disp_q8, status, frames=YAWED, W=LS.W):
    """Over the matched slots of `frames`: dict(n, rms_int, max_int, rms_ref, max_ref, edge_share) of disparity - fx b / Z
    in pixels, for the integer disparity of the keys and the refined one, and the share of matches with status 1.  The
    brute-force matcher's wrong matches (tens of pixels off, and refinement cannot move them by more than `search`) are in
    those figures; n_near, rms_int_near and rms_ref_near are the same over the matches whose integer disparity lies
    within NEAR_PX of the truth."""
    e_int, e_ref, edge = [], [], []
    for f in frames:
        i, j = S.matched(np.asarray(stereo_idx), kp_count, f)
        xl, yl, xr = S.positions(kp_keys, f, i, j, W)
        want = true_disparity(gt[f], xl, yl)
        e_int.append((xl - xr) - want)
        e_ref.append(np.asarray(disp_q8)[f, i] / 256.0 - want)
        edge.append(np.asarray(status)[f, i] == S.EDGE)
    e_int, e_ref, edge = np.concatenate(e_int), np.concatenate(e_ref), np.concatenate(edge)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    near = np.abs(e_int) <= NEAR_PX
    return dict(n=int(len(e_int)), rms_int=rms(e_int), max_int=float(np.abs(e_int).max()), rms_ref=rms(e_ref),
                max_ref=float(np.abs(e_ref).max()), edge_share=float(edge.mean()), n_near=int(near.sum()),
                rms_int_near=rms(e_int[near]), rms_ref_near=rms(e_ref[near]))
