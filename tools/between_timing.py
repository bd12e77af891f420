"""BetweenFactorPose3 stage and LM timing on the MI355X: vus_between_linearize / _assemble / _eval_step (device events,
median of --reps after a warm-up) and a whole LM (synchronised host clock) at
  - BASELINE.json configs[2] (synth.CONFIGS2_BA: 2000 keyframes, 50 k landmarks) without between factors, and with 2000
    odometry factors plus ~50 loop closures inside the landmark band;
  - a pose-only graph of 10 k poses (prior + odometry chain + in-band closures).
Each graph with between factors runs under the diagonal models and again with EVERY factor under a full-covariance model
(vus_between_factors.sqrt_info; keys ending in "_full"): the same sigmas turned by a seeded rotation of the tangent space
(condition 25).  The measurements stay as drawn, so the full graphs are other estimation problems and their trial counts
may differ; the stage times and the time per trial are what compares.  Writes one JSON.

    python tools/between_timing.py [--reps 20] [--json out.json]
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
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver, BetweenFactors, band_of  # noqa: E402
from visual_underwater_slam_amd.gtsam import Pose3  # noqa: E402


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


def between_set(rng, truth, pairs, noise=0.002):
    meas = []
    for a, b in pairs:
        m = Pose3.from_flat12(truth[a]).between(Pose3.from_flat12(truth[b])).retract(noise * rng.standard_normal(6))
        meas.append(m.flat12())
    sig = np.tile([0.01, 0.01, 0.01, 0.05, 0.05, 0.05], (len(pairs), 1))
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), np.array(meas), sig


def full_models(rng, sig):
    """sqrt_info [n, 6, 6] of the covariances Q diag(sig^2) Q^T, Q a seeded rotation per factor: upper Cholesky of cov^-1."""
    R = np.empty((len(sig), 6, 6))
    for f, s in enumerate(sig):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        R[f] = np.linalg.cholesky((Q / (s * s)) @ Q.T).T
    return R


def lm_seconds(sv, state):
    sv.optimize(*state)                      # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    *_, rep = sv.optimize(*state)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, rep


def stages(sv, poses, reps):
    sv.between_linearize(poses)
    out = {"linearize_ms": event_median(lambda: sv.between_linearize(poses), reps),
           "assemble_ms": event_median(sv.between_assemble, reps)}
    sv.dp.zero_()
    sv.new_poses.copy_(poses)
    out["eval_ms"] = event_median(lambda: sv.between_eval_step(poses), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    res = {"device": torch.cuda.get_device_name(0)}

    n_kf, n_lm, obs = synth.CONFIGS2_BA
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    nL = len(seq["points_gt"])
    args = (seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, nL, seq["K"], seq["sigma"])
    kw = dict(prior_pose=[0], prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None])
    state = (d(seq["poses_init"]), d(seq["points_init"]))
    prob0 = StereoBAProblem(*args, **kw)
    lm_band = band_of(prob0.pk)
    t0, rep0 = lm_seconds(StereoBASolver(prob0), state)
    res["configs2_plain"] = {"lm_s": t0, "iterations": rep0.iterations, "tries": rep0.tries, "band": prob0.band,
                             "lm_ms_per_try": 1e3 * t0 / max(rep0.tries, 1)}
    del prob0
    pairs = [(k - 1, k) for k in range(1, n_kf)]
    for _ in range(50):                                        # closures inside the landmark band
        i = int(rng.integers(0, n_kf - lm_band))
        pairs.append((i, i + int(rng.integers(2, max(lm_band, 3)))))
    bi, bj, bm, bs = between_set(rng, seq["poses_gt"], pairs)
    for key, R in (("configs2_between", None), ("configs2_between_full", full_models(rng, bs))):
        bf = BetweenFactors(bi, bj, bm, bs, n_kf, sqrt_info=R)
        prob = StereoBAProblem(*args, **kw, between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        st = stages(sv, state[0], a.reps)
        t1, rep1 = lm_seconds(sv, state)
        res[key] = {"factors": len(pairs), "band": prob.band, "lm_s": t1, "iterations": rep1.iterations,
                    "tries": rep1.tries, "lm_ms_per_try": 1e3 * t1 / max(rep1.tries, 1), **st}
        del sv, prob

    n = 10000
    truth = np.stack([Pose3.Expmap(np.r_[0, 0, 0.01 * k, 0.5 * k, 0.1 * np.sin(0.05 * k), 0]).flat12() for k in range(n)])
    pairs = [(k - 1, k) for k in range(1, n)] + [(k, k + 30) for k in range(0, n - 30, 100)]
    bi, bj, bm, bs = between_set(rng, truth, pairs)
    z = np.zeros(0, np.int32)
    init = np.stack([Pose3.from_flat12(T).retract(0.01 * rng.standard_normal(6)).flat12() for T in truth])
    init[0] = truth[0]
    pstate = (d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    for key, R in (("pose_graph_10k", None), ("pose_graph_10k_full", full_models(rng, bs))):
        bf = BetweenFactors(bi, bj, bm, bs, n, sqrt_info=R)
        prob = StereoBAProblem(z, z, np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=[0],
                               prior_T=truth[:1], prior_sigmas=np.full((1, 6), 1e-3), between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        st = stages(sv, pstate[0], a.reps)
        t2, rep2 = lm_seconds(sv, pstate)
        res[key] = {"poses": n, "factors": len(pairs), "band": prob.band, "lm_s": t2, "iterations": rep2.iterations,
                    "tries": rep2.tries, "status": rep2.status, "lm_ms_per_try": 1e3 * t2 / max(rep2.tries, 1), **st}
        del sv, prob
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
