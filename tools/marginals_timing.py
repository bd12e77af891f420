"""Marginal covariances at BASELINE.json configs[2] (synth.CONFIGS2_BA: 2000 keyframes, 50 k landmarks, 2.0 M factors):
the selected inversion of the band (vus_ba_band_selinv), the landmark covariances (vus_ba_point_covariance) and the whole
StereoBASolver.marginals() call (linearise, lambda = 0 Schur, one-sided factorisation, both of the above), each the median
of --reps runs after a warm-up.  The selected inversion is also reported as f64 rate against the MFMA peak (78.6 TF/s),
with its flop count 2 (6B)^2 48 per panel for the Sigma_RR X product plus the smaller terms.

    python tools/marginals_timing.py [--reps 10] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_underwater_slam_amd import synth, _lib  # noqa: E402
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver  # noqa: E402


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


def selinv_flops(n, band):
    """Multiply-adds x 2 of the panel recursion: X = L_RP L_PP^-1, Sigma_RR X, X^T Sigma_RP, L_PP^-T L_PP^-1."""
    f = 0.0
    for k0 in range(0, n, 8):
        r = 6 * max(0, min(n, k0 + 8 + band) - k0 - 8)
        f += 2 * r * 48 * 48 + 2 * r * r * 48 + 2 * r * 48 * 48 + 2 * 48 ** 3
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n_kf, n_lm, obs = synth.CONFIGS2_BA
    s = synth.ba_sequence(n_kf, n_lm, obs)
    nL = len(s["points_gt"])
    prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n_kf, nL, s["K"], s["sigma"], prior_pose=[0],
                           prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None])
    sv = StereoBASolver(prob)
    poses, points = torch.from_numpy(s["poses_gt"]).cuda(), torch.from_numpy(s["points_gt"]).cuda()
    m = sv.marginals(poses, points)                       # warm-up; leaves the factor in Sband
    nN, B = prob.n_nodes, prob.band
    nw = int(_lib.load().vus_ba_band_selinv_work_doubles(nN, B))
    work = torch.empty(nw, dtype=torch.float64, device="cuda")
    Sg = torch.empty_like(sv.Sband)
    p, st = _lib.ptr, _lib.current_stream_ptr()
    t_sel = event_median(lambda: _lib.call("vus_ba_band_selinv", p(sv.Sband), nN, B, p(Sg), p(work), nw, st), a.reps)
    t_pts = event_median(lambda: sv._point_cov(Sg), a.reps)
    walls = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sv.marginals(poses, points)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    fl = selinv_flops(nN, B)
    out = {"config": {"keyframes": n_kf, "landmarks": nL, "factors": prob.n_obs, "band": B},
           "selinv_ms": round(t_sel, 3), "selinv_gflop": round(fl / 1e9, 2),
           "selinv_tflops": round(fl / t_sel / 1e9, 2), "selinv_mfma_fraction": round(fl / t_sel / 1e9 / 78.6, 3),
           "point_cov_ms": round(t_pts, 3), "marginals_ms": round(float(np.median(walls)), 3),
           "pose_cov_min_eig": float(torch.linalg.eigvalsh(m.pose_cov).min().item())}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
