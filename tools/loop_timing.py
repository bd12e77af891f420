"""vus_stereo_pair_pose timing on the MI355X: one launch for 1, 64 and 512 keyframe pairs at 2000 keypoint slots, 256
hypotheses and 10 refit rounds (device events, median of --reps after a warm-up).  The tables are planted scenes of
tests/loop_ref.py at 1280 x 720 -- 300 true + 150 wrong matches per pair, and a second set with 1200 + 800 (every slot a
candidate) -- the same pair content repeated, so the time per pair is that of one known workload.  What it measures is
the kernel alone: matching the pairs (vus_hamming_match) is not included.  Writes one JSON.

    python tools/loop_timing.py [--reps 20] [--json out.json]
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
import loop_ref as R  # noqa: E402
from visual_underwater_slam_amd import _lib  # noqa: E402

K, N_HYP, REFINE, THRESHOLD, SEED = 2000, 256, 10, 2.0, 20261019


def event_median(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def launch(t, n_pairs):
    """A closure that runs the entry point on n_pairs copies of the table's pair 0 (frames 0 and 1)."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mt = d(np.tile(t["match_idx"][:1], (n_pairs, 1)))
    pa, pb = d(np.zeros(n_pairs, np.int32)), d(np.ones(n_pairs, np.int32))
    st, keys, cnt = d(t["stereo_idx"]), d(t["kp_keys"].view(np.int32)), d(t["kp_count"])
    out = torch.empty_like(mt)
    info = torch.empty((n_pairs, 6), dtype=torch.int32, device="cuda")
    T = torch.empty((n_pairs, 12), dtype=torch.float64, device="cuda")
    JtJ = torch.empty((n_pairs, 36), dtype=torch.float64, device="cuda")
    rss = torch.empty((n_pairs,), dtype=torch.float64, device="cuda")
    cam = np.ascontiguousarray(R.default_cam5(t["H"], t["W"]))
    keep = (mt, pa, pb, st, keys, cnt, out, info, T, JtJ, rss, cam)

    def fn():
        _lib.call("vus_stereo_pair_pose", mt.data_ptr(), pa.data_ptr(), pb.data_ptr(), st.data_ptr(), keys.data_ptr(),
                  cnt.data_ptr(), len(t["stereo_idx"]), n_pairs, K, t["H"], t["W"], cam.ctypes.data, THRESHOLD, N_HYP, SEED,
                  REFINE, T.data_ptr(), JtJ.data_ptr(), rss.data_ptr(), out.data_ptr(), info.data_ptr(),
                  _lib.current_stream_ptr())
    fn.keep, fn.info = keep, info
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "max_kp": K, "n_hyp": N_HYP, "refine_iters": REFINE, "reps": a.reps}
    for name, sizes in (("450_candidates", [(300, 150)]), ("2000_candidates", [(1200, 800)])):
        t = R.planted_tables(seed=71, K=K, sizes=sizes)
        row = {}
        for n_pairs in (1, 64, 512):
            fn = launch(t, n_pairs)
            ms = event_median(fn, a.reps)
            row[f"pairs_{n_pairs}_ms"] = ms
            row["info_pair0"] = fn.info[0].cpu().numpy().tolist()
        res[name] = row
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
