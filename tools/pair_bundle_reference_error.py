"""The "Closures" table of profiles/subpixel.md for the two-view refit of vus_stereo_pair_bundle: on the CPU oracle front
end's output (oracle/chain.frontend) for the closed track of tests/loop_scene.py, at 2 m and raised to 4 m, the same pairs
and inlier thresholds, with integer and with refined disparities -- the translation error of the left-image refit of
vus_stereo_pair_pose (tests/loop_ref.py, subpixel_ref.stereo_pair_pose_q8) and of the two-view refit started from it
(tests/pair_bundle_ref.py) at LoopClosureParams' defaults: sigma_uv 0.5 px, sigma_d 0.6 px for integer and 0.12 px for
refined disparities, gate 4, 10 rounds.  What comes out is reported, also where it shows no gain; no test asserts these
figures.  CPU only; prints one JSON line.

    python tools/pair_bundle_reference_error.py [--json out.json] [--write-profile]

--write-profile replaces the block between the reference-error markers of profiles/pair_bundle.md with the tables.
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
import pair_bundle_ref as B  # noqa: E402
import subpixel_ref as S  # noqa: E402
import subpixel_scene as SS  # noqa: E402
from oracle import chain, oracle as O  # noqa: E402
from visual_underwater_slam_amd import synth  # noqa: E402

BEGIN, END = "<!-- reference-error:begin -->", "<!-- reference-error:end -->"
PAIRS, THRESHOLDS = (LS.REVISIT, (1, 9), (2, 8)), (LS.THRESHOLD, 4.0)
SIGMA_UV, SIGMA_D, GATE, ITERS = 0.5, {"integer": 0.6, "refined": 0.12}, 4.0, 10


def measure(altitude):
    gt = SS.poses_at(altitude)
    frames = synth.scene_frames(gt, LS.H, LS.W)
    fe = chain.frontend(frames, LS.KP, 30, True)
    disp, _ = S.refine(frames.reshape(2 * LS.N_KF, LS.H, LS.W), LS.W, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"],
                       SS.HALF_WIN, SS.SEARCH)
    out = {}
    for a, b in PAIRS:
        pa, pb = np.array([a], np.int32), np.array([b], np.int32)
        fwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pa, 2 * pb, -1, 0, 0, LS.MATCH_DISTANCE)
        bwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], LS.W, 2 * pb, 2 * pa, -1, 0, 0, LS.MATCH_DISTANCE)
        t = LS.tables(O.cross_check(fwd, bwd), pa, pb, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"])
        truth = LS.relative(gt, a, b)
        for thr in THRESHOLDS:
            for kind in ("integer", "refined"):
                q8 = disp if kind == "refined" else None
                one = (L.stereo_pair_pose(t, thr, LS.N_HYP, synth.SEED, LS.REFINE) if q8 is None else
                       S.stereo_pair_pose_q8(t, q8, thr, LS.N_HYP, synth.SEED, LS.REFINE))
                two = B.stereo_pair_bundle(dict(t, match_idx=one["match_idx_out"]), one["T_ab"], one["info"], SIGMA_UV,
                                           SIGMA_D[kind], GATE, ITERS, q8)
                e1, r1 = L.pose_error(one["T_ab"][0], truth)
                e2, r2 = L.pose_error(two["T_ab"][0], truth)
                n_act = int(two["info"][0, 2])
                dof = 3 * n_act - 6
                out[f"{a}-{b} at {thr:g} px, {kind}"] = {
                    "left_mm": round(1e3 * e1, 1), "two_view_mm": round(1e3 * e2, 1), "left_mrad": round(1e3 * r1, 2),
                    "two_view_mrad": round(1e3 * r2, 2), "info_one": one["info"][0].tolist(), "info_two": two["info"][0].tolist(),
                    "scale": round(float(np.sqrt(two["chi2"][0] / dof)), 2) if dof > 0 else None}
    return out


def table(res):
    alts = list(res["altitudes"])
    rows = ["Translation error in mm, left-image refit / two-view refit behind it (final active points of stage one's inliers; "
            "s = sqrt(chi2 / (3 n - 6))):", "",
            "| Pair, inlier threshold, disparities | " + " | ".join(f"{a} m" for a in alts) + " |",
            "|---|" + "---|" * len(alts)]
    for key in res["altitudes"][alts[0]]:
        cells = []
        for a in alts:
            r = res["altitudes"][a][key]
            i2 = r["info_two"]
            what = f"{i2[2]} of {i2[0]}, s {r['scale']}" if i2[3] == 0 else f"status {i2[3]}"
            cells.append(f"{r['left_mm']} / {r['two_view_mm']} ({what})")
        a, rest = key.split(" at ")
        rows.append(f"| ({a.replace('-', ', ')}), {rest} | " + " | ".join(cells) + " |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--write-profile", action="store_true")
    a = ap.parse_args()
    res = {"image": [LS.H, LS.W], "max_features": LS.KP, "sigma_uv_px": SIGMA_UV, "sigma_disp_px": SIGMA_D, "gate": GATE,
           "iters": ITERS, "altitudes": {f"{alt:g}": measure(alt) for alt in (LS.ALTITUDE, SS.HIGH_ALTITUDE)}}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    if a.write_profile:
        path = os.path.join(ROOT, "profiles", "pair_bundle.md")
        txt = open(path).read()
        head, rest = txt.split(BEGIN)
        tail = rest.split(END)[1]
        with open(path, "w") as f:
            f.write(head + BEGIN + "\n" + table(res) + "\n" + END + tail)


if __name__ == "__main__":
    main()
