"""Monocular projection factors: what a mixed observation list costs the per-observation kernels on the MI355X.
vus_ba_linearize and vus_ba_eval_step (device events, median of --reps after a warm-up) at BASELINE.json configs[2]
(synth.CONFIGS2_BA: 2000 keyframes, 50 k landmarks, 2.0 M factors)
  - all stereo: the entry points and kernels of a graph without mono factors;
  - with --mono-frac of the observations (default 30 %, drawn by the seeded hash of synth.py) flagged mono: the `_mixed`
    entry points.  A flagged row keeps its (uL, v) and gets NaN in the unused middle slot; K_mono = (fx, fy, 0.5, cx, cy).
On a tree without mono support only the first is measured (the same script times the parent commit).  Writes one JSON.

    python tools/mono_timing.py [--reps 30] [--mono-frac 0.3] [--json out.json]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_underwater_slam_amd import synth, _lib  # noqa: E402
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver  # noqa: E402


def event_times(fn, reps):
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
    ts = np.sort(ts)
    return {"median_ms": float(np.median(ts)), "p10_ms": float(ts[len(ts) // 10]), "p90_ms": float(ts[(9 * len(ts)) // 10])}


def stages(prob, state, reps):
    sv = StereoBASolver(prob)
    poses, points = state
    sv.linearize(poses, points)
    sv.schur(1e-3); sv.band_solve(); sv.backsub()            # a real step for eval_step to evaluate
    out = {"entry_point": sv._loss_args("vus_ba_linearize")[0],
           "linearize": event_times(lambda: sv.linearize(poses, points), reps),
           "eval_step": event_times(lambda: sv.eval_step(poses, points), reps)}
    assert torch.isfinite(sv.scal).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mono-frac", type=float, default=0.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    n_kf, n_lm, obs = synth.CONFIGS2_BA
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    nL, n = len(seq["points_gt"]), len(seq["meas"])
    res = {"device": torch.cuda.get_device_name(0), "keyframes": n_kf, "landmarks": nL, "factors": n, "reps": a.reps}
    kw = dict(prior_pose=[0], prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None])
    state = (d(seq["poses_init"]), d(seq["points_init"]))
    res["all_stereo"] = stages(StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, nL, seq["K"],
                                               seq["sigma"], **kw), state, a.reps)
    if "mono" in inspect.signature(StereoBAProblem.__init__).parameters:
        mono = synth._hash_uniform(np.arange(n, dtype=np.int64), synth.SEED ^ 0x6D6F) < a.mono_frac
        meas = seq["meas"].copy()
        meas[mono, 1] = np.nan
        K = seq["K"]
        prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], meas, n_kf, nL, K, seq["sigma"], mono=mono,
                               mono_K=np.array([K[0], K[1], 0.5, K[3], K[4]]), mono_sigma=seq["sigma"], **kw)
        res["mixed"] = dict(stages(prob, state, a.reps), mono_frac=float(mono.mean()))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
