"""Inertial fixed-lag smoothing timing on the MI355X (include/vus_fixed_lag_nav.h), next to tools/fixed_lag_timing.py and with
its pose-only figures taken in the same run: device events, median of --reps after a warm-up, for
  - the marginalisation of (keyframes dropped, keyframes kept) = (1, 75) and (8, 75) in the per-keyframe-bias layout --
    vus_ba_band_marginalize on 3 nodes per keyframe with identity padding, then vus_nav_window_prior_compact -- against the
    pose-only (1, 224) and (8, 224);
  - the four stages of the nav_window_prior family at m = 75 (error, linearize, assemble, eval_step), against the pose-only
    family at m = 225;
  - eval_step on ONE matrix H of 1140 and of 3600 rows (10 and 104 MB) read as a nav prior of 76 / 240 keyframes and as a
    pose-only prior of 190 / 600 poses: the same row product in both families (profiles/fixed_lag_nav.md holds these next to
    the figures of a nav family that formed both products of eval_step in one sweep over H, which was not kept);
and, on the synchronised host clock, one whole BatchFixedLagSmoother.update at a 75-keyframe inertial window (the window
filled by one update, then the timed update that adds keyframe 75 and marginalises keyframe 0), split into pack / optimise /
marginalise as the smoother reports them.  Writes one JSON line.

    python tools/fixed_lag_nav_timing.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fixed_lag_timing import event_median, spd_band, marginalize_ms, family_ms  # noqa: E402
from visual_underwater_slam_amd import synth, _lib, gtsam, gtsam_unstable  # noqa: E402
from visual_underwater_slam_amd.ba import (StereoBAProblem, StereoBASolver, NavBiasBASolver, NavBiasFactors, NavWindowPrior,  # noqa: E402
                                           WindowPrior)
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, V, B, L  # noqa: E402

d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
F64 = dict(dtype=torch.float64, device="cuda")


def nav_marginalize_ms(rng, k, w, reps):
    """k keyframes dropped, w kept: 3 (k + w) nodes, band 3 w - 1, velocity nodes padded with an identity."""
    n, band = 3 * (k + w), 3 * w - 1
    Sb = spd_band(rng, n, band).reshape(n, band + 1, 6, 6)
    gs = rng.normal(size=(n, 6))
    for q in range(n):
        if q % 3 == 1:
            Sb[q, :, 3:, :] = 0.0
            Sb[q, 0, 3:, :3] = 0.0
            Sb[q, 0, :3, 3:] = 0.0
            Sb[q, 0, 3:, 3:] = np.eye(3)
            gs[q, 3:] = 0.0
        for s in range(1, min(q, band) + 1):
            if (q - s) % 3 == 1:
                Sb[q, s, :, 3:] = 0.0
    Sb, gs = d(Sb.reshape(n, band + 1, 36)), d(gs)
    H18, g18, quad = torch.empty((18 * w, 18 * w), **F64), torch.empty(18 * w, **F64), torch.empty(1, **F64)
    H, g = torch.empty((15 * w, 15 * w), **F64), torch.empty(15 * w, **F64)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().vus_ba_band_marginalize_work_doubles(n, band, 3 * k)), **F64)
    p, st = _lib.ptr, _lib.current_stream_ptr()

    def run():
        _lib.call("vus_ba_band_marginalize", p(Sb), n, band, p(gs), 3 * k, p(H18), p(g18), p(quad), p(status), p(work), st)
        _lib.call("vus_nav_window_prior_compact", p(H18), p(g18), w, p(H), p(g), st)
    ms = event_median(run, reps)
    assert int(status.item()) == 0 and bool(torch.isfinite(H).all())
    return ms


def _nav_solver(rng, m, H=None):
    n = m
    truth = np.stack([gtsam.Pose3.Expmap(np.r_[0, 0, 0.01 * k, 0.5 * k, 0.0, 0]).flat12() for k in range(n)])
    init = np.stack([gtsam.Pose3.from_flat12(T).retract(0.05 * rng.standard_normal(6)).flat12() for T in truth])
    if H is None:
        M = rng.normal(size=(15 * m, 15 * m))
        H = M @ M.T
    W = NavWindowPrior(0, truth, np.zeros((m, 3)), np.zeros((m, 6)), H, rng.normal(size=15 * m), 0.0, n)
    z = np.zeros(0, np.int32)
    prob = StereoBAProblem(z, z, np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=[0], prior_T=truth[:1],
                           prior_sigmas=np.full((1, 6), 1e-2), pose_stride=3, between_span=m)
    sv = NavBiasBASolver(prob, NavBiasFactors([0.0, 0.0, -9.81]), window_prior=W)
    state = (d(init), d(0.1 * rng.normal(size=(n, 3))), d(0.01 * rng.normal(size=(n, 6))))
    sv.linearize(state[0], torch.zeros((0, 3), **F64))
    sv.schur(0.0)
    sv.dp.zero_()
    sv.new_poses.copy_(state[0])
    sv.new_vels.copy_(state[1])
    sv.new_bias.copy_(state[2])
    return sv, state


def nav_family_ms(rng, m, reps):
    sv, state = _nav_solver(rng, m)
    return {"error_ms": event_median(lambda: sv._family_call("nav_window_prior", "error", lambda f: (*state, f.err, f.work)), reps),
            "linearize_ms": event_median(lambda: sv.nav_window_prior_linearize(*state), reps),
            "assemble_ms": event_median(sv.nav_window_prior_assemble, reps),
            "eval_ms": event_median(lambda: sv.nav_window_prior_eval_step(*state), reps)}


def same_matrix_both_families(rng, reps, rows=1140):
    """eval_step on the same H as a nav prior of rows / 15 keyframes and as a pose-only prior of rows / 6 poses."""
    M = rng.normal(size=(rows, rows))
    H = M @ M.T
    sv, state = _nav_solver(rng, rows // 15, H)
    one = event_median(lambda: sv.nav_window_prior_eval_step(*state), reps)
    m = rows // 6
    truth = np.stack([gtsam.Pose3.Expmap(np.r_[0, 0, 0.01 * k, 0.5 * k, 0.0, 0]).flat12() for k in range(m)])
    W = WindowPrior(0, truth, H, rng.normal(size=rows), 0.0, m)
    z = np.zeros(0, np.int32)
    prob = StereoBAProblem(z, z, np.zeros((0, 3)), m, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=[0], prior_T=truth[:1],
                           prior_sigmas=np.full((1, 6), 1e-2), between_span=m - 1)
    sp = StereoBASolver(prob, window_prior=W)
    poses = d(truth)
    sp.dp.zero_()
    sp.new_poses.copy_(poses)
    two = event_median(lambda: sp.window_prior_eval_step(poses), reps)
    return {"rows": rows, "H_MB": 8e-6 * rows * rows, "nav_eval_ms": one, "pose_only_eval_ms": two}


def smoother_update(n_window=75, n_lm=3000, obs=60):
    n = n_window + 1
    s = synth.nav_sequence(n, n_lm, obs, bias_walk_sigma=(2e-3, 2e-4), meas_sigma=1.0, dvl_sigma=0.1)
    K = gtsam.Cal3_S2Stereo(*s["K"])
    nm = gtsam.noiseModel
    noise = nm.Isotropic.Sigma(3, 1.0)
    params = gtsam.PreintegrationParams.MakeSharedU(9.81)
    first_seen = {}
    for q, j in zip(s["obs_pose"].tolist(), s["obs_point"].tolist()):
        first_seen[j] = min(first_seen.get(j, q), q)

    def chunk(lo, hi, known):
        g, theta, ts = gtsam.NonlinearFactorGraph(), gtsam.Values(), {}
        rows = np.nonzero((s["obs_pose"] >= lo) & (s["obs_pose"] < hi))[0]
        g.push_back(gtsam.StereoFactorBlock(s["meas"][rows], noise, [X(int(q)) for q in s["obs_pose"][rows]],
                                            [L(int(j)) for j in s["obs_point"][rows]], K))
        for i in range(lo, hi):
            if i == 0:
                g.push_back(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(s["poses_gt"][0]), nm.Diagonal.Sigmas(s["prior_sigmas"])))
                g.push_back(gtsam.PriorFactorVector(V(0), s["vels_gt"][0], nm.Isotropic.Sigma(3, 0.1)))
                g.push_back(gtsam.PriorFactorConstantBias(B(0), gtsam.imuBias.ConstantBias(), nm.Diagonal.Sigmas(np.array([0.1] * 3 + [0.01] * 3))))
            else:
                pim = gtsam.PreintegratedImuMeasurements(params, gtsam.imuBias.ConstantBias())
                for smp in s["imu"][i - 1]:
                    pim.integrateMeasurement(smp[:3], smp[3:6], smp[6])
                g.push_back(gtsam.ImuFactor(X(i - 1), V(i - 1), X(i), V(i), B(i - 1), pim))
                g.push_back(gtsam.BetweenFactorConstantBias(B(i - 1), B(i), gtsam.imuBias.ConstantBias(),
                                                            nm.Diagonal.Sigmas(np.array([2e-3] * 3 + [2e-4] * 3))))
                g.push_back(gtsam.DvlVelocityFactor(nm.Isotropic.Sigma(3, 0.1), V(i), X(i), s["dvl"][i]))
            theta.insert(X(i), gtsam.Pose3.from_flat12(s["poses_init"][i]))
            theta.insert(V(i), s["vels_gt"][i].copy())
            theta.insert(B(i), gtsam.imuBias.ConstantBias())
            for k in (X(i), V(i), B(i)):
                ts[k] = float(i)
        for j in sorted(set(s["obs_point"][rows].tolist()) - known):
            theta.insert(L(j), s["points_init"][j])
            ts[L(j)] = float(first_seen[j])
            known.add(j)
        return g, theta, ts
    sm = gtsam_unstable.BatchFixedLagSmoother(float(n_window) - 1.0)
    known = set()
    sm.update(*chunk(0, n_window, known))
    torch.cuda.synchronize()
    stats = sm.update(*chunk(n_window, n, known))
    return {"window": n_window, "observations": int(len(s["obs_pose"])), "lm_tries": sm.last_report.tries,
            **{k: v for k, v in stats.items() if k != "seconds"}, **{k + "_ms": 1e3 * v for k, v in stats["seconds"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0)}
    for k in (1, 8):
        res[f"nav_marginalize_{k}_75_ms"] = nav_marginalize_ms(rng, k, 75, a.reps)
        res[f"marginalize_{k}_224_ms"] = marginalize_ms(rng, k, 224, a.reps)
    res["nav_window_prior_m75"] = nav_family_ms(rng, 75, a.reps)
    res["window_prior_m225"] = family_ms(rng, 225, a.reps)
    res["row_product"] = [same_matrix_both_families(rng, a.reps, rows) for rows in (1140, 3600)]
    res["smoother_update"] = smoother_update()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
