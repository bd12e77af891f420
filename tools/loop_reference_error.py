"""What the numpy statement of vus_stereo_pair_pose (tests/loop_ref.py) makes of the CPU oracle front end's output
(oracle/chain.frontend) on the closed track of tests/loop_scene.py: the pose error of the revisit pair against ground
truth -- the figure tests/test_loop_sequence_gpu.py holds the GPU path to (within twice of it) -- and what becomes of the
pair without common ground.  CPU only; prints one JSON line.

    python tools/loop_reference_error.py [--json out.json]
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
import loop_scene as S  # noqa: E402
from oracle import chain, oracle as O  # noqa: E402
from visual_underwater_slam_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    gt = S.poses_gt()
    frames = synth.scene_frames(gt, S.H, S.W)
    fe = chain.frontend(frames, S.KP, 30, True)
    pa, pb = np.array([S.REVISIT[0], S.FALSE_PAIR[0]], np.int32), np.array([S.REVISIT[1], S.FALSE_PAIR[1]], np.int32)
    fwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], S.W, 2 * pa, 2 * pb, -1, 0, 0, S.MATCH_DISTANCE)
    bwd, _ = O.hamming_match(fe["desc"], fe["kp_keys"], fe["kp_count"], S.W, 2 * pb, 2 * pa, -1, 0, 0, S.MATCH_DISTANCE)
    t = S.tables(O.cross_check(fwd, bwd), pa, pb, fe["stereo_idx"], fe["kp_keys"], fe["kp_count"])
    mg = L.Margins()
    r = L.stereo_pair_pose(t, S.THRESHOLD, S.N_HYP, synth.SEED, S.REFINE, mg)
    et, er = L.pose_error(r["T_ab"][0], S.relative(gt, *S.REVISIT))
    res = {"image": [S.H, S.W], "max_features": S.KP, "keypoints": [int(v) for v in fe["kp_count"][:2]],
           "revisit": {"pair": list(S.REVISIT), "info": r["info"][0].tolist(), "error_m": et, "error_rad": er,
                       "rss": float(r["rss"][0])},
           "no_overlap": {"pair": list(S.FALSE_PAIR), "info": r["info"][1].tolist()},
           "margins": {"inlier": mg.inlier, "degenerate": mg.degenerate, "pivot": mg.pivot}}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
