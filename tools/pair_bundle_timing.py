"""vus_stereo_pair_bundle timing on the MI355X beside the vus_stereo_pair_pose call it follows, by the protocol of
tools/loop_timing.py: one launch of each for 1, 64 and 512 keyframe pairs at 2000 keypoint slots (device events, median of
--reps after a warm-up), on the same planted scenes of tests/loop_ref.py at 1280 x 720 -- 300 true + 150 wrong matches per
pair, and 1200 + 800 (every slot a candidate) -- the pair content repeated.  Stage one runs 256 hypotheses and 10 refit
rounds; stage two starts from its outputs (its final inliers are the candidates) and runs 10 rounds at sigma_uv 0.5 px,
sigma_d 0.6 px, gate 4.  Writes one JSON.

    python tools/pair_bundle_timing.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_ref as R  # noqa: E402
import loop_timing as LT  # noqa: E402
from visual_underwater_slam_amd import _lib  # noqa: E402

SIGMA_UV, SIGMA_D, GATE, ITERS = 0.5, 0.6, 4.0, 10


def launch(t, one, n_pairs):
    """A closure that runs the second stage on the outputs of loop_timing.launch's closure `one` (already run)."""
    mt, pa, pb, st, keys, cnt, out1, info1, T1, _, _, cam = one.keep
    T = torch.empty_like(T1)
    S = torch.empty((n_pairs, 36), dtype=torch.float64, device="cuda")
    chi2 = torch.empty((n_pairs,), dtype=torch.float64, device="cuda")
    pts = torch.empty((n_pairs, LT.K, 3), dtype=torch.float64, device="cuda")
    out = torch.empty_like(out1)
    info = torch.empty_like(info1)

    def fn():
        _lib.call("vus_stereo_pair_bundle", out1.data_ptr(), pa.data_ptr(), pb.data_ptr(), st.data_ptr(), keys.data_ptr(),
                  cnt.data_ptr(), len(t["stereo_idx"]), n_pairs, LT.K, t["H"], t["W"], cam.ctypes.data, None, T1.data_ptr(),
                  info1.data_ptr(), SIGMA_UV, SIGMA_D, GATE, ITERS, T.data_ptr(), S.data_ptr(), chi2.data_ptr(), pts.data_ptr(),
                  out.data_ptr(), info.data_ptr(), _lib.current_stream_ptr())
    fn.keep, fn.info = (T, S, chi2, pts, out, info), info
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "max_kp": LT.K, "n_hyp": LT.N_HYP, "refine_iters": LT.REFINE, "iters": ITERS,
           "sigma_uv_px": SIGMA_UV, "sigma_disp_px": SIGMA_D, "gate": GATE, "reps": a.reps}
    for name, sizes in (("450_candidates", [(300, 150)]), ("2000_candidates", [(1200, 800)])):
        t = R.planted_tables(seed=71, K=LT.K, sizes=sizes)
        row = {}
        for n_pairs in (1, 64, 512):
            one = LT.launch(t, n_pairs)
            row[f"pairs_{n_pairs}_stage_one_ms"] = LT.event_median(one, a.reps)
            two = launch(t, one, n_pairs)
            row[f"pairs_{n_pairs}_stage_two_ms"] = LT.event_median(two, a.reps)
            row["info_one_pair0"] = one.info[0].cpu().numpy().tolist()
            row["info_two_pair0"] = two.info[0].cpu().numpy().tolist()
        res[name] = row
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
