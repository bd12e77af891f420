"""Long loop closures as a low-rank correction of the band solve, timed on the MI355X (device events, median of --reps
after a warm-up, as tools/between_timing.py): per lambda trial of
  - BASELINE.json configs[2] (synth.CONFIGS2_BA: 2000 keyframes, 50 k landmarks) with 0, 1, 8 and 64 closures longer than
    the landmark band, spread over the trajectory, kept out of the band (BetweenFactors(max_span=landmark band));
  - the same graph with ONE such closure on the widened band (the default path; its Sband is about 1 GB), --wide-reps;
  - the pose graph of 10 k poses of DESIGN 7e with 1 and 64 long closures.
The trial (Schur + assemble, band solve, correction, back-substitution) and its parts: Schur + assemble, the one-sided
band solve, scatter + vus_ba_band_resolve, capacitance + correct.  The resolve's time per panel step is set against the
f64 MFMA issue rate (profiles/mfma_f64_rate_r04.txt).  The closure-free graph is also timed with the two-sided solve it
takes by default and with the one-sided solve a long set forces.  Writes one JSON line.

    python tools/long_closure_timing.py [--reps 20] [--wide-reps 5] [--skip-wide] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_underwater_slam_amd import synth, _lib  # noqa: E402
from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver, BetweenFactors, band_of  # noqa: E402
from visual_underwater_slam_amd.gtsam import Pose3  # noqa: E402
from between_timing import event_median, between_set  # noqa: E402

LAM = 1e-3


def spread(n, span, k):
    """k closures longer than `span` poses, both key orders, spread over a trajectory of n poses"""
    starts = np.linspace(0, n - span - 40, k).astype(int)
    return [(int(a), int(a + span + 1 + 7 * (c % 5))) if c % 2 else (int(a + span + 1 + 7 * (c % 5)), int(a))
            for c, a in enumerate(starts)]


def trial_parts(sv, state, reps):
    """per-trial times [ms] of a solver whose state has been linearised"""
    sv._lm_linearize(state)
    out = {"trial_ms": event_median(lambda: sv._lm_solve(LAM), reps),
           "assemble_ms": event_median(lambda: sv._assemble(LAM), reps)}

    def assemble_and_solve():
        sv._assemble(LAM)
        sv.band_solve()
    out["band_solve_ms"] = event_median(assemble_and_solve, reps) - out["assemble_ms"]
    out["band_mode"] = _lib.load().vus_ba_get_tuning(_lib.TUNE_LAST_BAND_MODE)
    out["split"] = bool(sv.use_split)
    if sv.C is not None:
        nN, B, p = sv.P.n_nodes, sv.P.band, _lib.ptr

        def resolve():
            sv._closure_call("vus_closure_scatter", lambda f: (sv.clo_rows, sv.clo_UZ))
            _lib.call("vus_ba_band_resolve", p(sv.Sband), nN, B, p(sv.clo_UZ), 6 * sv.C.n, None, 0, _lib.current_stream_ptr())

        def correct():
            sv._closure_call("vus_closure_capacitance", lambda f: (sv.clo_rows, sv.clo_UZ, sv.clo_C))
            sv._closure_call("vus_closure_correct", lambda f: (sv.clo_rows, sv.clo_UZ, sv.clo_C, sv.dp, 1, f.work))
        assemble_and_solve()                      # a valid factor in Sband; resolve does not modify it
        out["resolve_ms"] = event_median(resolve, reps)
        out["capacitance_correct_ms"] = event_median(correct, reps)
        panels = (nN + 7) // 8
        out["resolve_us_per_panel_step"] = 1e3 * out["resolve_ms"] / (2 * panels)
        # MFMAs of one workgroup's panel step: 3 row tiles x 6 band / 4 K steps, over 4 waves on 4 SIMDs
        out["mfma_per_wave_per_panel_step"] = 3 * (6 * B // 4) / 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wide-reps", type=int, default=5)
    ap.add_argument("--skip-wide", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    res = {"device": torch.cuda.get_device_name(0)}

    def keep(name, **values):              # every leg is reported as soon as it is measured
        res[name] = values
        print(f"{name}: {json.dumps(values)}", file=sys.stderr, flush=True)

    n_kf, n_lm, obs = synth.CONFIGS2_BA
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    nL = len(seq["points_gt"])
    args = (seq["obs_pose"], seq["obs_point"], seq["meas"], n_kf, nL, seq["K"], seq["sigma"])
    kw = dict(prior_pose=[0], prior_T=seq["poses_init"][:1], prior_sigmas=seq["prior_sigmas"][None])
    state = (d(seq["poses_init"]), d(seq["points_init"]))
    prob = StereoBAProblem(*args, **kw)
    span = band_of(prob.pk)
    sv = StereoBASolver(prob)
    keep("configs2_k0", band=prob.band, **trial_parts(sv, state, a.reps))
    sv.use_split = False                            # what a long set forces
    keep("configs2_k0_one_sided", **trial_parts(sv, state, a.reps))
    del sv, prob
    for k in (1, 8, 64):
        bi, bj, bm, bs = between_set(rng, seq["poses_gt"], spread(n_kf, span, k))
        bf = BetweenFactors(bi, bj, bm, bs, n_kf, max_span=span)
        prob = StereoBAProblem(*args, **kw, between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        keep(f"configs2_k{k}", band=prob.band, long=sv.C.n, **trial_parts(sv, state, a.reps))
        del sv, prob
    if not a.skip_wide:
        bi, bj, bm, bs = between_set(rng, seq["poses_gt"], [(1900, 50)])
        bf = BetweenFactors(bi, bj, bm, bs, n_kf)
        prob = StereoBAProblem(*args, **kw, between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        keep("configs2_k1_widened", band=prob.band, Sband_GB=sv.Sband.numel() * 8 / 1e9, **trial_parts(sv, state, a.wide_reps))
        del sv, prob
    del state
    torch.cuda.empty_cache()

    n = 10000
    truth = np.stack([Pose3.Expmap(np.r_[0, 0, 0.01 * k, 0.5 * k, 0.1 * np.sin(0.05 * k), 0]).flat12() for k in range(n)])
    init = np.stack([Pose3.from_flat12(T).retract(0.01 * rng.standard_normal(6)).flat12() for T in truth])
    init[0] = truth[0]
    pstate = (d(init), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    z = np.zeros(0, np.int32)
    for k in (0, 1, 64):
        pairs = [(i - 1, i) for i in range(1, n)] + [(i, i + 30) for i in range(0, n - 30, 100)] + (spread(n, 3000, k) if k else [])
        bi, bj, bm, bs = between_set(rng, truth, pairs)
        bf = BetweenFactors(bi, bj, bm, bs, n, max_span=30)
        prob = StereoBAProblem(z, z, np.zeros((0, 3)), n, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=[0],
                               prior_T=truth[:1], prior_sigmas=np.full((1, 6), 1e-3), between_span=bf.span)
        sv = StereoBASolver(prob, bf)
        keep(f"pose_graph_10k_k{k}", band=prob.band, **trial_parts(sv, pstate, a.reps))
        del sv, prob
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
