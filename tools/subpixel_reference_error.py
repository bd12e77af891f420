"""What the numpy statement of vus_stereo_refine (tests/subpixel_ref.py) makes of the CPU oracle front end's output
(oracle/chain.frontend) on the closed track of tests/loop_scene.py, at its own altitude (2 m, 19 px of disparity) and raised
to 4 m (9.6 px): over the yawed keyframes 1..9 the RMS and maximum of disparity - fx b / Z for the integer and the refined
disparities and the share of matches whose minimum sits at the edge of the search, and the pose error of the revisit
closure (0, 9) from integer disparities (tests/loop_ref.py) and from refined ones (subpixel_ref.stereo_pair_pose_q8).
tests/test_subpixel_sequence_gpu.py holds the GPU path to these figures.  CPU only; prints one JSON line.

    python tools/subpixel_reference_error.py [--json out.json] [--write-profile]

--write-profile replaces the block between the reference-error markers of profiles/subpixel.md with a table of the figures.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loop_ref as L  # noqa: E402
import loop_scene as LS  # noqa: E402
import subpixel_ref as S  # noqa: E402
import subpixel_scene as SS  # noqa: E402
from oracle import chain, oracle as O  # noqa: E402
from visual_underwater_slam_amd import synth  # noqa: E402

BEGIN, END = "<!-- reference-error:begin -->", "<!-- reference-error:end -->"


def measure(altitude):
    gt = SS.poses_at(altitude)
    frames = synth.scene_frames(gt, LS.H, LS.W)
    fe = chain.frontend(frames, LS.KP, 30, True)
    flat = frames.reshape(2 * LS.N_KF, LS.H, LS.W)
    disp, status = S.refine(flat, LS.W, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"], SS.HALF_WIN, SS.SEARCH)
    out = SS.disparity_errors(gt, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"], disp, status)
    def pair_tables(a, b):
        pa, pb = np.array([a], np.int32), np.array([b], np.int32)
        fwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pa, 2 * pb, -1, 0, 0, LS.MATCH_DISTANCE)
        bwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pb, 2 * pa, -1, 0, 0, LS.MATCH_DISTANCE)
        return LS.tables(O.cross_check(fwd, bwd), pa, pb, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"])

    def closure(t, truth, threshold):
        row = {}
        for name, r in (("integer", L.stereo_pair_pose(t, threshold, LS.N_HYP, synth.SEED, LS.REFINE)),
                        ("refined", S.stereo_pair_pose_q8(t, disp, threshold, LS.N_HYP, synth.SEED, LS.REFINE))):
            et, er = L.pose_error(r["T_ab"][0], truth)
            row[name] = {"info": r["info"][0].tolist(), "error_m": et, "error_rad": er}
        return row

    first = closure(pair_tables(*LS.REVISIT), LS.relative(gt, *LS.REVISIT), LS.THRESHOLD)
    out["closure_integer"], out["closure_refined"] = first["integer"], first["refined"]
    # for the record, not held by any test: other overlapping pairs and a wider inlier threshold; and what the estimator
    # makes of the TRUE disparities plus Gaussian noise (left-image refit, depths of keyframe a taken as exact)
    out["other_closures_mm"], out["noise_experiment_mm"] = {}, {}
    rng = np.random.default_rng(0)
    for a, b in (LS.REVISIT, (1, 9), (2, 8)):
        t, truth = pair_tables(a, b), LS.relative(gt, a, b)
        for thr in (LS.THRESHOLD, 4.0):
            c = closure(t, truth, thr)
            out["other_closures_mm"][f"{a}-{b} at {thr:g} px"] = [round(1e3 * c[k]["error_m"], 1) for k in ("integer", "refined")]
        _, _, x1, y1, _, x2, y2, _ = S.candidates_q8(t, 0, disp)
        d1, d2 = SS.true_disparity(gt[a], x1, y1), SS.true_disparity(gt[b], x2, y2)
        for sigma in (0.0, 0.05, 0.12, 0.2):
            errs = []
            for _ in range(4):
                o = L.pair_pose(x1, y1, d1 + sigma * rng.normal(size=len(d1)), x2, y2, d2 + sigma * rng.normal(size=len(d2)),
                                LS.CAM5, LS.THRESHOLD, LS.N_HYP, synth.SEED, 0, LS.REFINE)
                errs.append(round(1e3 * L.pose_error(o["T"], truth)[0], 1))
            out["noise_experiment_mm"][f"{a}-{b} sigma {sigma:g} px"] = errs
    return out


def table(res):
    rows = ["| Altitude | Disparity | Matches (kf 1..9) | Integer RMS / max (px) | Refined RMS / max (px) | Status 1 | "
            "Within 1.5 px: matches, integer RMS, refined RMS | Closure (0, 9) integer | Closure (0, 9) refined |",
            "|---|---|---|---|---|---|---|---|---|"]
    for alt, r in res["altitudes"].items():
        ci, cr = r["closure_integer"], r["closure_refined"]
        rows.append(f"| {alt} m | {r['disparity_px']:.1f} px | {r['n']} | {r['rms_int']:.3f} / {r['max_int']:.2f} | "
                    f"{r['rms_ref']:.3f} / {r['max_ref']:.2f} | {100 * r['edge_share']:.2f} % | {r['n_near']}, {r['rms_int_near']:.3f}, {r['rms_ref_near']:.3f} | "
                    f"{1e3 * ci['error_m']:.2f} mm, {ci['error_rad']:.2e} rad ({ci['info'][3]} inliers of {ci['info'][0]}) | "
                    f"{1e3 * cr['error_m']:.2f} mm, {cr['error_rad']:.2e} rad ({cr['info'][3]} inliers of {cr['info'][0]}) |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--write-profile", action="store_true")
    a = ap.parse_args()
    res = {"image": [LS.H, LS.W], "max_features": LS.KP, "half_win": SS.HALF_WIN, "search": SS.SEARCH, "altitudes": {}}
    for alt in (LS.ALTITUDE, SS.HIGH_ALTITUDE):
        r = measure(alt)
        r["disparity_px"] = float(LS.CAM5[0] * LS.CAM5[4] / alt)
        res["altitudes"][f"{alt:g}"] = r
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    if a.write_profile:
        path = os.path.join(ROOT, "profiles", "subpixel.md")
        txt = open(path).read()
        head, rest = txt.split(BEGIN)
        tail = rest.split(END)[1]
        with open(path, "w") as f:
            f.write(head + BEGIN + "\n" + table(res) + "\n" + END + tail)


if __name__ == "__main__":
    main()
