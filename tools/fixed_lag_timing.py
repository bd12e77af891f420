"""Fixed-lag smoothing timing on the MI355X (include/vus_fixed_lag.h): device events, median of --reps after a warm-up, for
  - vus_ba_band_marginalize at (n_drop, w) = (1, 224), (8, 224), (16, 240) on a random SPD band of half-bandwidth w - 1;
  - the three stages of the window_prior family at m = 225 (linearize, assemble, eval_step);
and, on the synchronised host clock, one whole BatchFixedLagSmoother.update at a 240-keyframe window (the window filled by
one update, then the timed update that adds keyframe 240 and marginalises keyframe 0), split into pack / optimise /
marginalise as the smoother reports them.  Writes one JSON line.

    python tools/fixed_lag_timing.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_underwater_slam_amd import synth, _lib, gtsam, gtsam_unstable  # noqa: E402
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver, WindowPrior  # noqa: E402
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L  # noqa: E402


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


def spd_band(rng, n, band):
    """A diagonally dominant random block band [n, band + 1, 36] (entry (i, s) = block (i, i - s))."""
    Sb = rng.normal(size=(n, band + 1, 6, 6))
    Sb[:, 0] = 0.5 * (Sb[:, 0] + Sb[:, 0].transpose(0, 2, 1)) + 12.0 * (2 * band + 1) * np.eye(6)
    return Sb.reshape(n, band + 1, 36)


def marginalize_ms(rng, k, w, reps):
    n, band = k + w, w - 1
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    Sb, gs = d(spd_band(rng, n, band)), d(rng.normal(size=(n, 6)))
    f64 = dict(dtype=torch.float64, device="cuda")
    H, g, quad = torch.empty((6 * w, 6 * w), **f64), torch.empty(6 * w, **f64), torch.empty(1, **f64)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().vus_ba_band_marginalize_work_doubles(n, band, k)), **f64)
    p, st = _lib.ptr, _lib.current_stream_ptr()
    ms = event_median(lambda: _lib.call("vus_ba_band_marginalize", p(Sb), n, band, p(gs), k, p(H), p(g), p(quad), p(status),
                                        p(work), st), reps)
    assert int(status.item()) == 0 and bool(torch.isfinite(H).all())
    return ms


def family_ms(rng, m, reps):
    n = m
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    truth = np.stack([gtsam.Pose3.Expmap(np.r_[0, 0, 0.01 * k, 0.5 * k, 0.0, 0]).flat12() for k in range(n)])
    init = np.stack([gtsam.Pose3.from_flat12(T).retract(0.05 * rng.standard_normal(6)).flat12() for T in truth])
    M = rng.normal(size=(6 * m, 6 * m))
    W = WindowPrior(0, truth, M @ M.T, rng.normal(size=6 * m), 0.0, n)
    z = np.zeros(0, np.int32)
    prob = StereoBAProblem(z, z, np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=[0], prior_T=truth[:1],
                           prior_sigmas=np.full((1, 6), 1e-2), between_span=m - 1)
    sv = StereoBASolver(prob, window_prior=W)
    poses = d(init)
    sv.linearize(poses, torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    sv.schur(0.0)
    out = {"linearize_ms": event_median(lambda: sv.window_prior_linearize(poses), reps),
           "assemble_ms": event_median(sv.window_prior_assemble, reps)}
    sv.dp.zero_()
    sv.new_poses.copy_(poses)
    out["eval_ms"] = event_median(lambda: sv.window_prior_eval_step(poses), reps)
    return out


def smoother_update(n_window=240, n_lm=8000, obs=60):
    n = n_window + 1
    seq = synth.ba_sequence(n, n_lm, obs, meas_sigma=1.0)
    K = gtsam.Cal3_S2Stereo(*seq["K"])
    noise = gtsam.noiseModel.Isotropic.Sigma(3, 1.0)
    odo_noise = gtsam.noiseModel.Diagonal.Sigmas(np.array([0.005] * 3 + [0.02] * 3))
    gt = [gtsam.Pose3.from_flat12(T) for T in seq["poses_gt"]]
    first_seen = {}
    for p, j in zip(seq["obs_pose"].tolist(), seq["obs_point"].tolist()):
        first_seen.setdefault(j, p)

    def chunk(lo, hi, known):
        g, theta, ts = gtsam.NonlinearFactorGraph(), gtsam.Values(), {}
        rows = np.nonzero((seq["obs_pose"] >= lo) & (seq["obs_pose"] < hi))[0]
        g.push_back(gtsam.StereoFactorBlock(seq["meas"][rows], noise, [X(int(p)) for p in seq["obs_pose"][rows]],
                                            [L(int(j)) for j in seq["obs_point"][rows]], K))
        for i in range(lo, hi):
            g.push_back(gtsam.PriorFactorPose3(X(0), gt[0], gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])) if i == 0
                        else gtsam.BetweenFactorPose3(X(i - 1), X(i), gt[i - 1].between(gt[i]), odo_noise))
            theta.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
            ts[X(i)] = float(i)
        for j in sorted(set(seq["obs_point"][rows].tolist()) - known):
            theta.insert(L(j), seq["points_init"][j])
            ts[L(j)] = float(first_seen[j])
            known.add(j)
        return g, theta, ts
    sm = gtsam_unstable.BatchFixedLagSmoother(float(n_window) - 1.0)
    known = set()
    sm.update(*chunk(0, n_window, known))
    torch.cuda.synchronize()
    stats = sm.update(*chunk(n_window, n, known))
    return {"window": n_window, "observations": int(len(seq["obs_pose"])), "lm_tries": sm.last_report.tries,
            **{k: v for k, v in stats.items() if k != "seconds"}, **{k + "_ms": 1e3 * v for k, v in stats["seconds"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0)}
    for k, w in ((1, 224), (8, 224), (16, 240)):
        res[f"marginalize_{k}_{w}_ms"] = marginalize_ms(rng, k, w, a.reps)
    res["window_prior_m225"] = family_ms(rng, 225, a.reps)
    res["smoother_update"] = smoother_update()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
