"""Sub-pixel stereo disparities on the front end's own output, on the closed track of tests/loop_scene.py (ten rendered
keyframes at 640 x 360) at its own altitude of 2 m and raised to 4 m: refine_stereo equals the numpy statement on the GPU
front end's tables, the refined disparities are nearer the rendered geometry than the integer ones, few minima sit at the
edge of the search, the 4 m revisit closure is nearer the truth with them, and run_sequence takes them through both graph
builders and the loop closures -- and is unchanged without the new argument.

The recorded figures.  tools/subpixel_reference_error.py runs the numpy statements on the CPU oracle front end's output
for the same frames (profiles/subpixel.md).  Over the yawed keyframes 1..9, disparity - fx b / Z:

    altitude   matches   integer RMS   refined RMS   status 1   within 1.5 px: matches, integer RMS, refined RMS
    2 m        10411     3.0946 px     3.0119 px     0.17 %     9873, 0.5985 px, 0.1195 px
    4 m         7318     0.9335 px     0.6592 px     0.01 %     7025, 0.5967 px, 0.1225 px

(the all-match figures carry the brute-force matcher's wrong matches, tens of pixels off, which a search of +-5 columns
cannot move), and the revisit closure (0, 9) at 4 m is 281.5 mm off with integer disparities and 192.8 mm with refined
ones.  At 2 m the closure is 4.8 mm off with integer and 9.4 mm with refined disparities -- printed, not asserted: on a
plane at one depth the integer disparities that pass the inlier test are all the same integer, a constant bias without
noise, which the left-image refit tolerates better than 0.1-0.2 px of noise.  The GPU front end is bit-exact against the oracle, so the GPU figures
should EQUAL the recorded ones; they are held to 25 % of them."""
import numpy as np
import pytest
import torch

import loop_ref as L
import loop_scene as LS
import subpixel_ref as S
import subpixel_scene as SS
from visual_underwater_slam_amd import synth

pytestmark = pytest.mark.gpu

RECORDED = {2.0: dict(rms_int=3.0946, rms_ref=3.0119, edge_share=0.0017, rms_int_near=0.5985, rms_ref_near=0.1195),
            4.0: dict(rms_int=0.9335, rms_ref=0.6592, edge_share=0.0001, rms_int_near=0.5967, rms_ref_near=0.1225,
                      closure_int_m=0.28146, closure_ref_m=0.19282)}
MARGIN = 0.25
EDGE_CAP = 0.10
IDEAL_ROUNDING_PX = 12.0 ** -0.5            # RMS of a uniform error of +-0.5 px: what integer disparities could reach at best


@pytest.fixture(scope="module", params=[2.0, 4.0])
def track(gpu, request):
    from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend
    from visual_underwater_slam_amd.sequence import SEQUENCE_PARAMS
    alt = request.param
    gt = SS.poses_at(alt)
    frames = synth.scene_frames(gt, LS.H, LS.W, xp=torch, device="cuda").contiguous()
    fe = StereoOrbFrontend(LS.H, LS.W, max_frames=LS.N_KF, params=ImageProcessorParams(max_features=LS.KP, **SEQUENCE_PARAMS))
    res = fe.process(frames)
    disp, status = fe.refine_stereo(res, frames, SS.HALF_WIN, SS.SEARCH)
    torch.cuda.synchronize()
    host = dict(frames=frames.cpu().numpy().reshape(2 * LS.N_KF, LS.H, LS.W), sidx=res.stereo_idx.cpu().numpy(),
                keys=res.kp_keys.cpu().numpy().view(np.uint32), cnt=res.kp_count.cpu().numpy(), disp=disp.cpu().numpy(),
                status=status.cpu().numpy())
    return dict(alt=alt, gt=gt, fe=fe, res=res, disp=disp, status=status, host=host)


def test_refine_equals_the_reference_on_the_front_ends_tables(track):
    h = track["host"]
    want_d, want_s = S.refine(h["frames"], LS.W, h["sidx"], h["keys"], h["cnt"], SS.HALF_WIN, SS.SEARCH)
    assert (want_s != S.NONE).sum() > 5000
    assert np.array_equal(h["disp"], want_d) and np.array_equal(h["status"], want_s)


def test_refined_disparities_are_nearer_the_geometry_and_few_sit_at_the_edge(track):
    h, rec = track["host"], RECORDED[track["alt"]]
    e = SS.disparity_errors(track["gt"], h["sidx"], h["keys"], h["cnt"], h["disp"], h["status"])
    print(f"altitude {track['alt']} m, keyframes 1..9: {e}")
    assert e["rms_ref"] < e["rms_int"], e                               # the relation
    assert e["edge_share"] <= EDGE_CAP, e                                # the condition
    assert e["rms_ref_near"] < IDEAL_ROUNDING_PX < e["rms_int_near"], e  # sub-pixel: better than ideal rounding could be
    for k, v in rec.items():
        if not k.startswith("closure"):
            assert abs(e[k] - v) <= MARGIN * v + 5e-5, (k, e[k], v)      # 5e-5: the recorded values carry four decimals


def test_the_revisit_closure_with_refined_disparities(track):
    fe, res = track["fe"], track["res"]
    pa, pb = [LS.REVISIT[0]], [LS.REVISIT[1]]
    midx = fe.match_keyframes(res, pa, pb, max_distance=LS.MATCH_DISTANCE)
    whole = fe.relative_poses(res, pa, pb, midx, LS.CAM5, LS.THRESHOLD, LS.N_HYP, synth.SEED, LS.REFINE)
    fine = fe.relative_poses(res, pa, pb, midx, LS.CAM5, LS.THRESHOLD, LS.N_HYP, synth.SEED, LS.REFINE, disparity=track["disp"])
    torch.cuda.synchronize()
    h = track["host"]
    t = LS.tables(midx.cpu().numpy(), pa, pb, h["sidx"], h["keys"], h["cnt"])
    ref = S.stereo_pair_pose_q8(t, h["disp"], LS.THRESHOLD, LS.N_HYP, synth.SEED, LS.REFINE)
    assert np.array_equal(fine.info.cpu().numpy(), ref["info"]) and np.array_equal(fine.match_idx_out.cpu().numpy(), ref["match_idx_out"])
    assert np.abs(fine.T_ab.cpu().numpy() - ref["T_ab"]).max() <= 1e-8 * np.abs(ref["T_ab"]).max()
    truth = LS.relative(track["gt"], *LS.REVISIT)
    ei, _ = L.pose_error(whole.T_ab[0].cpu().numpy(), truth)
    er, _ = L.pose_error(fine.T_ab[0].cpu().numpy(), truth)
    print(f"altitude {track['alt']} m, closure {LS.REVISIT}: {1e3 * ei:.2f} mm with integer disparities (info "
          f"{whole.info[0].tolist()}), {1e3 * er:.2f} mm with refined ones (info {fine.info[0].tolist()})")
    assert fine.info[0, 4].item() == 0
    if track["alt"] == SS.HIGH_ALTITUDE:
        rec = RECORDED[track["alt"]]
        assert er < ei, (er, ei)
        assert abs(ei - rec["closure_int_m"]) <= MARGIN * rec["closure_int_m"], (ei, rec)
        assert abs(er - rec["closure_ref_m"]) <= MARGIN * rec["closure_ref_m"], (er, rec)


def test_run_sequence_with_subpixel_on_both_builders_and_unchanged_without(gpu):
    from oracle import chain
    from visual_underwater_slam_amd import gtsam, sequence
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X
    n = 4
    sc = synth.scene_sequence(n, LS.H, LS.W)
    frames = torch.from_numpy(sc["frames"]).cuda()
    args = (frames, sc["poses_init"], sc["imu"], sc["dvl"])
    # without the argument: the stereo factors of the oracle chain, bit for bit -- what run_sequence has always produced
    r0, _, s0 = sequence.run_sequence(*args, disparity_sign=1)
    r1, _, s1 = sequence.run_sequence(*args, disparity_sign=1, subpixel=None)
    fe = chain.frontend(sc["frames"], 2000, **sequence.SEQUENCE_PARAMS)
    cam = np.array([*synth.INTRINSIC, -synth.BASELINE_M, 1920, 1080, 0.0])
    fac = chain.factors(fe, sc["poses_init"], cam, sc["K"], sequence.GATE_PX)
    for s in (s0, s1):
        assert not any(k.startswith("stereo_") for k in s)
        for k in ("obs_frame", "obs_id", "obs_meas"):
            assert np.array_equal(s["factors"][k].cpu().numpy(), fac[k]), k
    p0 = np.stack([r0.atPose3(X(i)).flat12() for i in range(n)])
    assert np.array_equal(p0, np.stack([r1.atPose3(X(i)).flat12() for i in range(n)]))
    # with it: the stages appear, uR changes and nothing else of the measurements does, LM runs on both builders
    prm = sequence.LoopClosureParams(min_gap=1, radius_m=5.0, max_angle_rad=1.0, max_per_keyframe=1)
    for bulk in (True, False):
        for lc in (None, prm):
            r2, seq2, s2 = sequence.run_sequence(*args, disparity_sign=1, bulk=bulk, subpixel=sequence.SubpixelParams(),
                                                 loop_closure=lc)
            assert {"stereo_disparity", "stereo_refine_status"} <= set(s2)
            d, st = s2["stereo_disparity"], s2["stereo_refine_status"]
            assert d.dtype == torch.int32 and st.dtype == torch.uint8 and tuple(d.shape) == tuple(st.shape) == (n, 2000)
            assert torch.equal(s2["ids"], s0["ids"])
            f0, f2 = s0["feats"].cpu().numpy(), s2["feats"].cpu().numpy()
            assert np.array_equal(f0[..., [0, 1, 3]], f2[..., [0, 1, 3]]) and not np.array_equal(f0[..., 2], f2[..., 2])
            p2 = np.stack([r2.atPose3(X(i)).flat12() for i in range(n)])
            assert np.isfinite(p2).all() and not np.array_equal(p2, p0)
            if lc is not None:
                btw = [f for f in seq2.graph._factors if isinstance(f, gtsam.BetweenFactorPose3)]
                assert len(btw) == int(s2["loop_accepted"].sum()) >= 1
            if bulk:
                u = s2["factors_ungated"]["obs_meas"].cpu().numpy()
                u0 = s0["factors_ungated"]["obs_meas"].cpu().numpy()
                assert u.shape == u0.shape and np.array_equal(u[:, [0, 2]], u0[:, [0, 2]]) and (np.abs(u[:, 1] - u0[:, 1]) <= 3 * 4.5 + 1e-9).all()   # |s*| <= 4, |q| <= 128; 3 units per pixel
                assert set(s2) - set(s0) == {"stereo_disparity", "stereo_refine_status"} | ({"loop_pairs", "loop_result", "loop_accepted"} if lc else set())
