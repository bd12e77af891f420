"""One IMU bias per keyframe (NavBiasBASolver, pose_stride 3) against one shared bias (NavBASolver, pose_stride 2) on the
same data: one LM iteration, the whole optimize(), and the stages of one trial (linearise, Schur step + inertial assembly,
band solve), median of --reps runs each.  Prints one JSON line.

    python tools/nav_bias_timing.py [--keyframes 2000] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from visual_underwater_slam_amd import synth  # noqa: E402
from visual_underwater_slam_amd.ba import (StereoBAProblem, NavBASolver, NavFactors, NavBiasBASolver,  # noqa: E402
                                           NavBiasFactors, LMParams)
from visual_underwater_slam_amd.gtsam.imu import Preintegrator  # noqa: E402

ACC_COV, GYRO_COV, INT_COV = np.eye(3) * 9e-08, np.eye(3) * 1.2184696791468346e-07, np.eye(3) * 1e-07


def build(s, stride):
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    pims, Ws = [], []
    for samples in s["imu"]:
        pre = Preintegrator(np.zeros(6), ACC_COV, GYRO_COV, INT_COV)
        for smp in samples:
            pre.integrate(smp[:3], smp[3:6], smp[6])
        pims.append(pre.packed()); Ws.append(pre.whitening().reshape(-1))
    imu = (np.arange(n - 1), np.arange(1, n), np.array(pims), np.array(Ws))
    dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
    vpr = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
    prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                           prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=stride)
    if stride == 2:
        return NavBASolver(prob, NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr))
    sig = np.tile(np.repeat([2e-3, 2e-4], 3), (n - 1, 1))
    return NavBiasBASolver(prob, NavBiasFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vpr,
                                                bbetween=(np.arange(n - 1), np.arange(1, n), np.zeros((n - 1, 6)), sig),
                                                bprior=([0], np.zeros((1, 6)), np.repeat([[0.1, 0.01]], 3, 1))))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def measure(sv, s, bias0, reps):
    n = len(s["poses_gt"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poses, vels, bias, points = d(s["poses_init"]), d(np.zeros((n, 3))), d(bias0), d(s["points_init"])
    lam = 1e-3
    sv.optimize(poses, vels, bias, points, LMParams(maxIterations=1))        # warm-up (code objects, allocator)
    r = {"n_nodes": sv.P.n_nodes, "band": sv.P.band, "split_solve": bool(sv.use_split)}
    r["linearize_ms"] = timed(lambda: (sv.linearize(poses, points), sv.nav_linearize(poses, vels, bias)), reps)
    r["schur_assemble_ms"] = timed(lambda: (sv.schur(lam), sv.nav_assemble(lam)), reps)

    def solve():
        sv.schur(lam); sv.nav_assemble(lam); sv.nav_solve(lam)
    r["band_solve_ms"] = round(timed(solve, reps) - r["schur_assemble_ms"], 3)
    r["lm_iteration_ms"] = timed(lambda: sv.optimize(poses, vels, bias, points, LMParams(maxIterations=1)), reps)
    reports = []
    r["optimize_ms"] = timed(lambda: reports.append(sv.optimize(poses, vels, bias, points)[4]), reps)
    rep = reports[-1]
    r.update(iterations=rep.iterations, tries=rep.tries, final_error=rep.final_error)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    n = a.keyframes
    s = synth.nav_sequence(n, 20 * n, 40, bias_walk_sigma=(2e-3, 2e-4))
    out = {"keyframes": n, "landmarks": len(s["points_gt"]), "observations": len(s["obs_pose"]), "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    out["shared_bias"] = measure(build(s, 2), s, np.zeros(6), a.reps)
    out["per_keyframe_bias"] = measure(build(s, 3), s, np.zeros((n, 6)), a.reps)
    sh, pk = out["shared_bias"], out["per_keyframe_bias"]
    out["ratio"] = {k: round(pk[k] / sh[k], 3) for k in ("linearize_ms", "schur_assemble_ms", "band_solve_ms",
                                                          "lm_iteration_ms", "optimize_ms")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
