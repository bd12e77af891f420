"""Per-stage LM times of the stereo BA at BASELINE.json configs[2] (synth.CONFIGS2_BA: 2000 keyframes, 2.0 M factors),
Gaussian against a robust noise model (default Cauchy k = 2.3849): linearise, step evaluation, Schur, band solve and
back-substitution, each the median of --reps launches timed with HIP events after a warm-up, plus a full LM solve
(iterations, trials, wall time) of the same problem with and without ~3 % injected outliers.

    python tools/robust_lm_timing.py [--reps 20] [--loss cauchy] [--k 2.3849] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_underwater_slam_amd import synth  # noqa: E402
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver  # noqa: E402


def stage_times(sv, poses, points, reps):
    stages = {"linearize": lambda: sv.linearize(poses, points), "schur": lambda: sv.schur(1e-3),
              "band_solve": sv.band_solve, "backsub": sv.backsub, "eval_step": lambda: sv.eval_step(poses, points),
              "error": lambda: sv.error(poses, points)}
    sv.linearize(poses, points)
    out = {}
    for name, fn in stages.items():
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
        out[name] = round(float(np.median(ts)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loss", default="cauchy")
    ap.add_argument("--k", type=float, default=2.3849)
    ap.add_argument("--outliers", type=float, default=0.03)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {}
    for tag, frac in (("clean", 0.0), ("outliers", a.outliers)):
        seq = synth.ba_sequence(*synth.CONFIGS2_BA)
        if frac > 0:
            synth.inject_outliers(seq, frac)
        nP, nL = len(seq["poses_gt"]), len(seq["points_gt"])
        for name, loss in (("gaussian", None), (a.loss, (a.loss, a.k))):
            prob = StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], nP, nL, seq["K"], seq["sigma"],
                                   prior_pose=[0], prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None],
                                   loss=loss)
            sv = StereoBASolver(prob)
            poses, points = torch.from_numpy(seq["poses_init"]).cuda(), torch.from_numpy(seq["points_init"]).cuda()
            r = {"stages_ms": stage_times(sv, poses, points, a.reps) if tag == "clean" else None}
            sv.optimize(poses, points)                                  # warm
            p, pt, rep = sv.optimize(poses, points)
            rms = float(np.sqrt(np.mean(np.sum((p.cpu().numpy()[:, 9:] - seq["poses_gt"][:, 9:]) ** 2, 1))))
            r.update(iterations=rep.iterations, outer=rep.outer, tries=rep.tries, status=rep.status,
                     lm_seconds=round(rep.seconds, 4), rms_t_m=rms, n_obs=prob.n_obs)
            res[f"{tag}/{name}"] = r
            print(tag, name, json.dumps(r), flush=True)
            del sv, prob
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
