"""One decision log for every reference Levenberg-Marquardt of the tests.

`replay(stages, **LMParams fields)` is GTSAM's iterate / tryLambda / checkConvergence with a fixed lambda factor -- the loop of
ba.py's StereoBASolver._levenberg_marquardt, of oracle.ba_lm_optimize and of the `lm` / `lm_optimize` of the numpy
references -- over a small stages object, and it keeps what those loops throw away: every trial, rejected ones included,
with its damping, its three errors, the model fidelity, the decisions taken and a copy of the trial state, and per
linearisation the decreases the convergence test saw.  The arithmetic is not here: an adapter hands the stage functions
a reference already has to the replay.

A stages object has
    error() -> float                  nonlinear error at the current state
    linearize() -> float              linearise at the current state; the linear system's error at delta = 0
    solve(lam) -> int                 the damped step of the last linearisation; 0, or the band solve's status word
    eval() -> (lin1, new1, state)     linearised error at the step, nonlinear error at the trial state, the trial state
    accept()                          the trial state becomes the current state
    state() -> tuple of arrays        the current state
"""
import math

import numpy as np

EPS = 2.220446049250313e-16
DEFAULTS = dict(lambdaInitial=1e-5, lambdaFactor=10.0, lambdaUpperBound=1e5, lambdaLowerBound=0.0, minModelFidelity=1e-3,
                maxIterations=100, relativeErrorTol=1e-5, absoluteErrorTol=1e-5, errorTol=0.0)
# LMParams field -> keyword of oracle.ba_lm_optimize, BAPort.optimize, between_ref / nav_bias_ref.lm_optimize
ORACLE_NAMES = dict(lambdaInitial="lambda_initial", lambdaFactor="lambda_factor", lambdaUpperBound="lambda_upper",
                    lambdaLowerBound="lambda_lower", minModelFidelity="min_model_fidelity", maxIterations="max_iterations",
                    relativeErrorTol="rel_tol", absoluteErrorTol="abs_tol", errorTol="error_tol")
REPORT_KEYS = ("iterations", "outer", "tries", "status")


def oracle_params(params):
    """LMParams-named parameters under the oracle's keyword names"""
    return {ORACLE_NAMES[k]: v for k, v in params.items()}


def _copy(state):
    return tuple(np.array(x, dtype=np.float64, copy=True) for x in state)


def replay(stages, **params):
    """Returns the log: the report of oracle.ba_lm_optimize (iterations, outer, tries, status, initial_error, final_error,
    final_lambda, err_hist, lambda_hist) plus
      trials  one dict per linear solve: outer (index of its linearisation), lam, status, lin0, lin1, new1, fidelity
              (None where GTSAM does not form it), rel_cost = |cost_change| / current (None likewise), lin_change,
              accepted, stop_search, outcome ("A" accepted, "R" rejected and lambda raised, "S" search abandoned by
              stop_search, "U" lambda reached its upper bound) and state, a copy of the trial state (None: no step)
      outers  one dict per linearisation: error, lam (both after it), rel_dec, abs_dec, converged
      state   the final state."""
    prm = dict(DEFAULTS)
    unknown = set(params) - set(prm)
    assert not unknown, unknown
    prm.update(params)
    log = {"iterations": 0, "outer": 0, "tries": 0, "status": 1, "err_hist": [], "lambda_hist": [], "trials": [], "outers": [],
           "params": prm}
    lam = prm["lambdaInitial"]
    current = stages.error()
    log["initial_error"] = current
    if current <= prm["errorTol"] or prm["maxIterations"] <= 0:       # before the first iterate(): the state is untouched
        log.update(status=0 if current <= prm["errorTol"] else 1, final_error=current, final_lambda=lam, state=_copy(stages.state()))
        return log
    while log["iterations"] < prm["maxIterations"]:
        lin0 = stages.linearize()
        new_error, stop_search, accepted = current, False, False
        while True:
            status = stages.solve(lam)
            t = {"outer": log["outer"], "lam": lam, "status": status, "lin0": lin0, "lin1": None, "new1": None, "fidelity": None,
                 "rel_cost": None, "lin_change": None, "state": None}
            log["tries"] += 1
            success = False
            if status == 0:
                lin1, new1, trial_state = stages.eval()
                t.update(lin1=lin1, new1=new1, state=_copy(trial_state))
                if math.isfinite(lin1) and math.isfinite(new1):
                    lin_change = lin0 - lin1
                    t["lin_change"] = lin_change
                    if lin_change >= 0.0:
                        cost_change = current - new1
                        t["rel_cost"] = abs(cost_change) / current
                        if lin_change > EPS * lin0:
                            t["fidelity"] = cost_change / lin_change
                            success = t["fidelity"] > prm["minModelFidelity"]
                        if abs(cost_change) < prm["relativeErrorTol"] * current:
                            stop_search = True
                        if success:
                            stages.accept()
                            new_error = new1
            t.update(accepted=success, stop_search=stop_search)
            log["trials"].append(t)
            if success:
                lam = max(prm["lambdaLowerBound"], lam / prm["lambdaFactor"])
                accepted = True
                t["outcome"] = "A"
                break
            if stop_search:
                t["outcome"] = "S"
                break
            lam *= prm["lambdaFactor"]
            if lam >= prm["lambdaUpperBound"]:
                log["status"] = 2
                t["outcome"] = "U"
                break
            t["outcome"] = "R"
        log["err_hist"].append(new_error)
        log["lambda_hist"].append(lam)
        log["outer"] += 1
        log["iterations"] += int(accepted)
        abs_dec = current - new_error
        rel_dec = abs_dec / current
        converged = new_error <= prm["errorTol"] or rel_dec <= prm["relativeErrorTol"] or abs_dec <= prm["absoluteErrorTol"]
        log["outers"].append({"error": new_error, "lam": lam, "rel_dec": rel_dec, "abs_dec": abs_dec, "converged": converged})
        current = new_error
        if log["status"] == 2:
            break
        if converged:
            log["status"] = 0
            break
        if not math.isfinite(current):
            break
    log.update(final_error=current, final_lambda=lam, state=_copy(stages.state()))
    return log


def outcomes(log):
    """the decision sequence: (lambda, outcome, status word) of every trial"""
    return [(t["lam"], t["outcome"], t["status"]) for t in log["trials"]]


def _gap(a, b):
    """relative distance of a from the threshold b"""
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def narrowest_margin(log):
    """The smallest relative distance of any compared quantity of the log from its threshold: fidelity from
    minModelFidelity, |cost_change| from relativeErrorTol * current, the decreases and the error of every linearisation
    from relativeErrorTol, absoluteErrorTol and errorTol, and lin_change from zero (relative to lin0).  Returns (margin,
    what), what naming the narrowest comparison."""
    prm = log["params"]
    found = []
    for k, t in enumerate(log["trials"]):
        if t["lin_change"] is not None:
            found.append((abs(t["lin_change"]) / abs(t["lin0"]), f"trial {k}: lin_change against 0"))
        if t["fidelity"] is not None:
            found.append((_gap(t["fidelity"], prm["minModelFidelity"]), f"trial {k}: fidelity {t['fidelity']:.6g}"))
        if t["rel_cost"] is not None:
            found.append((_gap(t["rel_cost"], prm["relativeErrorTol"]), f"trial {k}: |cost_change| / current {t['rel_cost']:.6g}"))
    for k, o in enumerate(log["outers"]):
        found.append((_gap(o["rel_dec"], prm["relativeErrorTol"]), f"linearisation {k}: relative decrease {o['rel_dec']:.6g}"))
        found.append((_gap(o["abs_dec"], prm["absoluteErrorTol"]), f"linearisation {k}: absolute decrease {o['abs_dec']:.6g}"))
        found.append((_gap(o["error"], prm["errorTol"]), f"linearisation {k}: error {o['error']:.6g}"))
    return min(found) if found else (math.inf, "no decision")


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def value_differences(log_a, log_b):
    """Largest relative differences between two logs of the same decisions: {"lin0": of the first linearisation, a kernel's
    output on bit-identical input; "scalars": lin1 and new1 of every trial and lin0 of every later linearisation, all of
    them evaluated at a state that a solve produced -- a comparison that lets states differ by a solve's tolerance cannot
    ask more of a function of those states; "state": every trial state, each array by its largest entry, and the final
    state}."""
    assert outcomes(log_a) == outcomes(log_b)
    out = {"lin0": 0.0, "scalars": 0.0, "state": 0.0}
    for a, b in zip(log_a["trials"], log_b["trials"]):
        key = "scalars" if a["outer"] else "lin0"
        out[key] = max(out[key], relerr(a["lin0"], b["lin0"]))
        if b["lin1"] is None or b["status"] != 0:
            continue
        out["scalars"] = max(out["scalars"], relerr(a["lin1"], b["lin1"]), relerr(a["new1"], b["new1"]))
        if a["state"] is not None and b["state"] is not None:
            out["state"] = max([out["state"]] + [relerr(x, y) for x, y in zip(a["state"], b["state"])])
    out["state"] = max([out["state"]] + [relerr(x, y) for x, y in zip(log_a["state"], log_b["state"])])
    return out


def same_report(log, rep, err_rtol=0.0):
    """`rep` (a report dict of an oracle or reference LM) tells what the log tells: counts, status and lambda_hist exactly,
    err_hist within err_rtol"""
    assert {k: log[k] for k in REPORT_KEYS} == {k: rep[k] for k in REPORT_KEYS}, (log, rep)
    assert list(log["lambda_hist"]) == list(rep["lambda_hist"]) and log["final_lambda"] == rep["final_lambda"]
    assert len(log["err_hist"]) == len(rep["err_hist"])
    assert np.allclose(log["err_hist"], rep["err_hist"], rtol=err_rtol, atol=0), (log["err_hist"], rep["err_hist"])
    assert np.isclose(log["final_error"], rep["final_error"], rtol=err_rtol, atol=0)


def log_from_report(rep, state, **params):
    """The log of an oracle LM that returns its trials (oracle.ba_lm_optimize, oracle.nav_lm_optimize: `trials` = (lambda,
    lin0, lin1, new1, status) per linear solve) in replay()'s shape, so that outcomes(), narrowest_margin() and
    value_differences() read it; the trial states, which the C loop does not return, are None.  The outcome of a trial
    follows from the report alone: the trial after an accepted or abandoned one starts a linearisation."""
    prm = dict(DEFAULTS)
    prm.update(params)
    log = {k: rep[k] for k in REPORT_KEYS + ("initial_error", "final_error", "final_lambda", "err_hist", "lambda_hist")}
    log.update(trials=[], outers=[], params=prm, state=_copy(state))
    current, k = rep["initial_error"], 0
    for o in range(rep["outer"]):
        new_error = rep["err_hist"][o]
        while True:
            lam, lin0, lin1, new1, status = rep["trials"][k]
            last = k + 1 == len(rep["trials"]) or rep["trials"][k + 1][0] != lam * prm["lambdaFactor"] or \
                rep["trials"][k + 1][1] != lin0
            ok = status == 0 and math.isfinite(lin1) and math.isfinite(new1) and lin0 - lin1 >= 0.0
            t = {"outer": o, "lam": lam, "status": status, "lin0": lin0, "lin1": lin1, "new1": new1, "state": None,
                 "lin_change": lin0 - lin1 if status == 0 else None, "rel_cost": abs(current - new1) / current if ok else None,
                 "fidelity": (current - new1) / (lin0 - lin1) if ok and lin0 - lin1 > EPS * lin0 else None}
            t["accepted"] = last and new_error == new1 and new_error != current
            t["outcome"] = "R" if not last else "A" if t["accepted"] else "U" if (rep["status"] == 2 and o + 1 == rep["outer"]) else "S"
            log["trials"].append(t)
            k += 1
            if last:
                break
        abs_dec = current - new_error
        log["outers"].append({"error": new_error, "lam": rep["lambda_hist"][o], "rel_dec": abs_dec / current, "abs_dec": abs_dec,
                              "converged": None})
        current = new_error
    assert k == len(rep["trials"]) == rep["tries"]
    return log


# -- adapters -------------------------------------------------------------------------------------------------------------
class OracleStereoStages:
    """the scalar oracle's stage functions ba_linearize, ba_schur, ba_band_solve, ba_backsub, ba_eval_step"""

    def __init__(self, O, P, band, poses, points):
        self.O, self.P, self.band = O, P, int(band)
        self.cur = _copy((poses, points))

    def state(self):
        return self.cur

    def error(self):
        return self.O.ba_error(self.P, *self.cur)

    def linearize(self):
        self.lin = self.O.ba_linearize(self.P, *self.cur)
        return self.lin["err"]

    def solve(self, lam):
        self.sch = self.O.ba_schur(self.P, self.band, lam, self.lin)
        self.dp, status, _ = self.O.ba_band_solve(self.sch["Sband"], self.sch["gs"])
        return status

    def eval(self):
        dl = self.O.ba_backsub(self.P, self.lin, self.sch["Vinv"], self.dp)
        npo, npt, lin1, new1 = self.O.ba_eval_step(self.P, *self.cur, self.dp, dl)
        self.trial = (npo, npt)
        return lin1, new1, self.trial

    def accept(self):
        self.cur = self.trial


class PortStages:
    """oracle.ba_port.BAPort's stage methods: multi-threaded kernels and LAPACK's band Cholesky"""

    def __init__(self, port, poses, points):
        self.port = port
        self.cur = _copy((poses, points))

    def state(self):
        return self.cur

    def error(self):
        return self.port.error(*self.cur)

    def linearize(self):
        return self.port.linearize(*self.cur)

    def solve(self, lam):
        self.port.schur(lam)
        self.dp, ok = self.port.band_solve()
        return 0 if ok else 1

    def eval(self):
        self.port.backsub(self.dp)
        npo, npt, lin1, new1 = self.port.eval_step(*self.cur, self.dp)
        self.trial = (npo, npt)
        return lin1, new1, self.trial

    def accept(self):
        self.cur = self.trial


class RobustStages:
    """robust_ref.RobustBA and the classes built on it (SensorBA, MonoBA, PointPriorBA, PoseMeasBA): error, linearize,
    solve(lin, lam), eval_step -- the stages RobustBA.lm drives"""

    def __init__(self, R, poses, points):
        self.R = R
        self.cur = _copy((poses, points))

    def state(self):
        return self.cur

    def error(self):
        return self.R.error(*self.cur)

    def linearize(self):
        self.lin = self.R.linearize(*self.cur)
        return self.lin["err"]

    def solve(self, lam):
        try:
            self.step = self.R.solve(self.lin, lam)
        except np.linalg.LinAlgError:
            return 1
        return 0

    def eval(self):
        npo, npt, lin1, new1 = self.R.eval_step(*self.cur, *self.step)
        self.trial = (npo, npt)
        return lin1, new1, self.trial

    def accept(self):
        self.cur = self.trial


class NavBiasStages:
    """nav_bias_ref's dense LM, one bias per keyframe: lm_trial() (the trial nav_bias_ref.lm_optimize runs) and the error
    functions.  state = (poses, vels, biases, points)."""

    def __init__(self, O, s, P, G, poses, vels, biases, points, cholesky=False):
        self.O, self.s, self.P, self.G, self.cholesky = O, s, P, G, cholesky
        self.cur = _copy((poses, vels, biases, points))

    def state(self):
        return self.cur

    def error(self):
        import nav_bias_ref
        return nav_bias_ref.total_error(self.O, self.P, self.G, *self.cur)

    def linearize(self):
        import nav_bias_ref
        poses, vels, biases, points = self.cur
        return self.O.ba_linearize(self.P, poses, points)["err"] + nav_bias_ref.inertial_system(self.O, self.G, poses, vels, biases)[2]

    def solve(self, lam):
        import nav_bias_ref
        try:
            self.lin0, self.lin1, self.new1, self.trial = nav_bias_ref.lm_trial(self.O, self.s, self.P, self.G, *self.cur, lam, self.cholesky)
        except np.linalg.LinAlgError:
            return 1
        return 0

    def eval(self):
        return self.lin1, self.new1, self.trial

    def accept(self):
        self.cur = self.trial


# -- starts -----------------------------------------------------------------------------------------------------------------
def neighbour_start(poses_init, seed=1, turned=(), S=None):
    """Every keyframe but the first starts at the initial pose of the keyframe before or after it: the step Gauss-Newton
    proposes from there raises the error and LM has to reject trials.  In the lawn-mower sweep of synth.ba_sequence a
    neighbour across a line turn faces the other way, and that is what makes the start rough; on a straight track the
    keyframes `turned` get the same half turn about the optical axis of their camera (at pose o S with an extrinsic S)."""
    n = len(poses_init)
    sign = np.random.default_rng(seed).integers(0, 2, n - 1) * 2 - 1
    out = np.array(poses_init, dtype=np.float64, copy=True)
    out[1:] = poses_init[np.clip(np.arange(1, n) + sign, 0, n - 1)]
    for i in turned:
        import sensor_ref
        cam = out[i].copy() if S is None else sensor_ref.compose(out[i], S)
        cam[:9] = (cam[:9].reshape(3, 3) @ np.diag([-1.0, -1.0, 1.0])).reshape(-1)
        out[i] = cam if S is None else sensor_ref.compose(cam, sensor_ref.inverse(S))
    return out


# -- the stereo scene and the table of cases ------------------------------------------------------------------------------
_scene = {}


def stereo_scene(O):
    """synth.ba_sequence(12, 60, 30) -- 12 keyframes, 50 landmarks, 357 observations, band 11 -- as the oracle problem, with
    the three starts of the table.  Computed once and shared (read only)."""
    if not _scene:
        import torch
        from visual_underwater_slam_amd import synth, ba_pack
        s = synth.ba_sequence(12, 60, 30)
        nL = len(s["points_gt"])
        pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                       torch.from_numpy(s["meas"]), 12, nL)
        st = ba_pack.build_structure(pk)
        P = O.BAProblem(pk, s["K"], s["sigma"], (np.array([0], np.int32), s["poses_gt"][:1], s["prior_sigmas"][None]))
        assert (nL, pk["n_obs"], st["band"]) == (50, 357, 11)
        shape = s["points_init"].shape
        starts = {"neighbour": (neighbour_start(s["poses_init"]), s["points_init"]),
                  "points+N(0,1)": (s["poses_init"], s["points_init"] + np.random.default_rng(0).normal(0.0, 1.0, shape)),
                  "points+N(0,0.3)": (s["poses_init"], s["points_init"] + np.random.default_rng(0).normal(0.0, 0.3, shape))}
        _scene.update(seq=s, pk=pk, st=st, P=P, band=st["band"], starts=starts)
    return _scene


# name -> (start, LMParams fields, the reference outcome: tries, outer, accepted steps, status, lambda_hist)
STEREO_CASES = {
    "defaults": ("neighbour", dict(maxIterations=3), (13, 3, 3, 1, [100.0, 100.0, 100.0])),
    "upper-bound": ("neighbour", dict(lambdaUpperBound=1e-2), (3, 1, 0, 2, [0.01])),
    "stop-search": ("neighbour", dict(minModelFidelity=0.9, relativeErrorTol=0.5), (9, 1, 0, 0, [1e3])),
    "factor-3": ("neighbour", dict(lambdaFactor=3.0, maxIterations=3), (21, 3, 3, 1, None)),
    "lower-bound-free": ("neighbour", dict(lambdaInitial=1e3, lambdaLowerBound=10.0, maxIterations=6),
                         (11, 6, 6, 1, [100.0, 100.0, 100.0, 1e3, 1e3, 100.0])),
    # lambdaInitial 1e3 alone is accepted at once from this start (fidelity 0.846); with the next row's minModelFidelity the
    # two trials at 1e3 and 1e4 are rejected and lambda reaches its upper bound
    "upper-bound-from-1e3": ("points+N(0,1)", dict(lambdaInitial=1e3, lambdaLowerBound=10.0, minModelFidelity=0.9),
                             (2, 1, 0, 2, [1e5])),
    "fidelity-0.9": ("points+N(0,1)", dict(minModelFidelity=0.9), (10, 1, 0, 2, [1e5])),
    "lower-bound-binds": ("points+N(0,0.3)", dict(lambdaInitial=1e3, lambdaLowerBound=10.0, maxIterations=6),
                          (6, 6, 6, 1, [100.0, 10.0, 10.0, 10.0, 10.0, 10.0])),
    "error-tol": ("points+N(0,0.3)", dict(errorTol=1e3), (2, 2, 2, 0, None)),
    "absolute-tol": ("points+N(0,0.3)", dict(absoluteErrorTol=1e4), (2, 2, 2, 0, None)),
    "max-iterations-0": ("neighbour", dict(maxIterations=0), (0, 0, 0, 1, [])),
    "error-tol-above-start": ("neighbour", dict(errorTol=1e9), (0, 0, 0, 0, [])),
}
_logs = {}


def stereo_logs(O, name):
    """(scalar-oracle replay, BAPort replay, BAPort) of one case of the table, computed once and shared (read only)"""
    if name not in _logs:
        from oracle.ba_port import BAPort
        sc = stereo_scene(O)
        start, prm, _ = STEREO_CASES[name]
        port = BAPort(sc["P"], sc["st"])
        _logs[name] = (replay(OracleStereoStages(O, sc["P"], sc["band"], *sc["starts"][start]), **prm),
                       replay(PortStages(port, *sc["starts"][start]), **prm), port)
    return _logs[name]


# -- the other stereo configurations: each on the 16-keyframe scene of its family's own LM test, with its own reference ----
class BetweenFixesBA:
    """Mixin over pose_meas_ref.PoseMeasBA (made by between_fixes_ba()): the BetweenFactorPose3 terms of between_ref
    (factors, system, linear_error) added to the error, to the reduced camera system (`pose_H`, `pose_g` of the
    linearisation, which RobustBA.solve adds) and to the linearised error."""

    def error(self, poses, points):
        import between_ref
        return super().error(poses, points) + between_ref.error(self.O, self.B, np.asarray(poses, np.float64).reshape(-1, 12))

    def linearize(self, poses, points):
        import between_ref
        lin = super().linearize(poses, points)
        H, g, e, self._btw_fac = between_ref.system(self.O, self.B, np.asarray(poses, np.float64).reshape(-1, 12), self.nP)
        lin.update(pose_H=H, pose_g=g, btw_err=e, err=lin["err"] + e)
        return lin

    def linear_error(self, dp, dl):
        import between_ref
        return super().linear_error(dp, dl) + between_ref.linear_error(self._btw_fac, np.asarray(dp).reshape(-1))


def between_fixes_ba(*args, between, **kw):
    import pose_meas_ref
    cls = type("BetweenFixesBA", (BetweenFixesBA, pose_meas_ref.PoseMeasBA), {})
    R = cls(*args, **kw)
    R.B = between
    return R


CAUCHY = (2, 2.3849)
# name -> (mono fraction, stereo outliers, stereo loss, with extrinsic, with between + landmark priors + fixes)
FAMILIES = {"cauchy": (0.0, 0.10, CAUCHY, False, False), "extrinsic": (0.0, 0.0, (0, 0.0), True, False),
            "mono": (0.4, 0.0, (0, 0.0), False, False), "between+priors+fixes": (0.0, 0.0, (0, 0.0), False, True)}
FAMILY_PARAMS = {"defaults": dict(maxIterations=3), "upper-bound": dict(lambdaUpperBound=1e-2)}
_families = {}


def family_case(O, name):
    """The scene, the factor sets, the numpy reference and the neighbour start of one configuration, computed once and
    shared (read only).  `gpu()` builds the StereoBAProblem and StereoBASolver of the same graph."""
    if name in _families:
        return _families[name]
    import torch
    from visual_underwater_slam_amd import ba_pack
    import between_ref
    import mono_problem
    import pose_meas_ref
    import sensor_ref
    mono_frac, outliers, loss, with_sensor, with_terms = FAMILIES[name]
    S = sensor_ref.extrinsic() if with_sensor else None
    seq = mono_problem.mixed_sequence(mono_frac=mono_frac, n_kf=16, n_lm=80, outliers=outliers)
    if S is not None:
        seq = sensor_ref.body_sequence(seq, S)
    nP, nL = len(seq["poses_gt"]), len(seq["points_gt"])
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]),
                                   torch.from_numpy(seq["meas"]), nP, nL)
    perm = pk["perm"].numpy().astype(np.int64)
    B = Q = M = None
    if with_terms:      # odometry in both key orders and two closures; priors on six landmarks; fixes of every kind
        from visual_underwater_slam_amd.gtsam import Pose3
        pairs = [(i - 1, i) if i % 2 else (i, i - 1) for i in range(1, nP)] + [(nP - 1, 2), (4, 11)]
        T = [Pose3.from_flat12(x) for x in seq["poses_gt"]]
        noise = 0.02 * np.random.default_rng(5).standard_normal((len(pairs), 6))
        B = between_ref.BetweenSet([a for a, _ in pairs], [b for _, b in pairs],
                                   np.array([T[a].between(T[b]).retract(e).flat12() for (a, b), e in zip(pairs, noise)]),
                                   np.tile((0.01, 0.01, 0.01, 0.05, 0.05, 0.05), (len(pairs), 1)))
        idx = np.array([nL - 1, 20, 0, 33, 20, 7])
        Q = (idx, seq["points_gt"][idx] + np.array([0.1, -0.2, 0.3]), np.tile((0.3, 0.05, 0.7), (len(idx), 1)))
        M, _ = pose_meas_ref.fix_set(seq["poses_gt"])
    priors = (np.array([0]), seq["poses_gt"][:1], seq["prior_sigmas"][None])
    R = between_fixes_ba(O, pk, seq["K"], seq["sigma"], *loss, S, np.asarray(seq["mono"])[perm], seq["mono_K"], seq["mono_sigma"],
                         priors, point_priors=Q, pose_meas=M, between=B if B is not None else between_ref.BetweenSet(
                             [], [], np.zeros((0, 12)), np.ones((0, 6))))
    # the twin of the pair the noise floor is measured on: the same class on the rows in REVERSE order, so that every sum over
    # observations (V, gl, Hpp, gp, the Schur complement, the errors) runs the other way round
    rev = dict(n_poses=nP, n_points=nL, n_obs=R.nO, obs_pose=R.op[::-1].copy(), obs_point=R.ol[::-1].copy(), meas=R.meas[::-1].copy())
    R2 = between_fixes_ba(O, rev, seq["K"], seq["sigma"], *loss, S, np.asarray(seq["mono"])[perm][::-1].copy(), seq["mono_K"],
                          seq["mono_sigma"], priors, point_priors=Q, pose_meas=M, between=R.B)
    start = (neighbour_start(seq["poses_init"], turned=(3, 8, 13), S=S), seq["points_init"])

    def gpu():
        from visual_underwater_slam_amd import ba
        prob = ba.StereoBAProblem(seq["obs_pose"], seq["obs_point"], seq["meas"], nP, nL, seq["K"], seq["sigma"], prior_pose=[0],
                                  prior_T=seq["poses_gt"][:1], prior_sigmas=seq["prior_sigmas"][None],
                                  loss=loss if loss[0] else None, body_P_sensor=S, mono=seq["mono"], mono_K=seq["mono_K"],
                                  mono_sigma=seq["mono_sigma"], between_span=B.span if B is not None else 0)
        assert np.array_equal(prob.pk["perm"].cpu().numpy().astype(np.int64), perm)
        return prob, ba.StereoBASolver(prob, between=None if B is None else B.device(nP),
                                       point_priors=None if Q is None else ba.PointPriors(*Q, nL),
                                       pose_meas=None if M is None else M.device(nP))
    _families[name] = dict(seq=seq, R=R, R2=R2, start=start, gpu=gpu, logs={}, between=B)
    return _families[name]


def family_logs(O, name, which):
    """(the replay of FAMILY_PARAMS[which] over the family's reference from its start, the same over its reversed-rows
    twin), computed once"""
    c = family_case(O, name)
    if which not in c["logs"]:
        c["logs"][which] = tuple(replay(RobustStages(R, *c["start"]), **FAMILY_PARAMS[which]) for R in (c["R"], c["R2"]))
    return c["logs"][which]


# -- the smallest sequence that takes the two-sided band solve ---------------------------------------------------------------
_split = {}


def split_case(O):
    """synth.ba_sequence(72, 432, 30, line_len=72, kf_step=1.5): one line of 72 keyframes 1.5 m apart, band 4, so that
    n_nodes = 2 band + 64 exactly; the plain neighbour start is 1.5 m off and rejects trials as it is"""
    if not _split:
        import torch
        from visual_underwater_slam_amd import synth, ba_pack
        n = 72
        s = synth.ba_sequence(n, 6 * n, 30, line_len=n, kf_step=1.5)
        pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                       torch.from_numpy(s["meas"]), n, len(s["points_gt"]))
        st = ba_pack.build_structure(pk)
        assert st["band"] == 4
        P = O.BAProblem(pk, s["K"], s["sigma"], (np.array([0], np.int32), s["poses_gt"][:1], s["prior_sigmas"][None]))
        _split.update(seq=s, st=st, P=P, start=(neighbour_start(s["poses_init"]), s["points_init"]), logs={})
    return _split


def split_logs(O, which):
    """(scalar-oracle replay, BAPort replay) of FAMILY_PARAMS[which] on split_case(), computed once"""
    c = split_case(O)
    if which not in c["logs"]:
        from oracle.ba_port import BAPort
        c["logs"][which] = (replay(OracleStereoStages(O, c["P"], c["st"]["band"], *c["start"]), **FAMILY_PARAMS[which]),
                            replay(PortStages(BAPort(c["P"], c["st"]), *c["start"]), **FAMILY_PARAMS[which]))
    return c["logs"][which]


# -- the inertial layouts: synth.nav_sequence(10, 200, 50), the sequence of the full-graph smoke run -----------------------
_inertial = {}


def inertial_case(O):
    """The 10-keyframe inertial sequence with a pose prior on X(0), ImuFactors between consecutive keyframes, DVL on 1..9
    and a zero prior on V(0): the oracle's shared-bias graph (P, N) and nav_bias_ref's per-keyframe-bias graph (P, G) --
    their references support no between factors, landmark priors or pose fixes -- from the neighbour start with
    keyframes 4 and 5 turned, zero velocities and zero biases.  (With keyframes 3 and 8 turned the dense system of the second
    linearisation is close to singular at small lambda: LU and Cholesky of it disagree in the second digit, and a
    comparison of values there would compare nothing.)  `gpu(kind)` builds the NavBASolver / NavBiasBASolver."""
    if not _inertial:
        import torch
        from visual_underwater_slam_amd import synth, ba_pack
        import nav_bias_ref
        n = 10
        s = synth.nav_sequence(n, 200, 50)
        nL = len(s["points_gt"])
        pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                       torch.from_numpy(s["meas"]), n, nL)
        pims, Ws = nav_bias_ref.preintegrate(s)
        imu = (np.arange(n - 1), np.arange(1, n), pims, Ws)
        dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
        vprior = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
        P, G = nav_bias_ref.make_graph(O, s)
        N = O.NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vprior)
        poses = neighbour_start(s["poses_init"], turned=(4, 5))
        starts = {"nav": (poses, np.zeros((n, 3)), np.zeros(6), s["points_init"]),
                  "navb": (poses, np.zeros((n, 3)), np.zeros((n, 6)), s["points_init"])}

        def gpu(kind):
            from visual_underwater_slam_amd import ba
            if kind == "navb":
                return nav_bias_ref.solver(s, G)
            prob = ba.StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                                      prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=2)
            return prob, ba.NavBASolver(prob, ba.NavFactors(s["gravity"], imu=imu, dvl=dvl, vprior=vprior))
        _inertial.update(seq=s, P=P, N=N, G=G, starts=starts, gpu=gpu, logs={})
    return _inertial


def inertial_logs(O, kind, which):
    """FAMILY_PARAMS[which] from inertial_case()'s start, (log, twin): kind "navb" = the replay over nav_bias_ref's dense LM
    and its twin with the Cholesky solve; "nav" = the log of oracle.nav_lm_optimize (from the trials its report returns; no
    trial states) -- the C loop is the shared-bias graph's one reference, so its twin is None.  Computed once."""
    c = inertial_case(O)
    if (kind, which) not in c["logs"]:
        prm = FAMILY_PARAMS[which]
        if kind == "nav":
            *state, rep = O.nav_lm_optimize(c["P"], c["N"], *c["starts"]["nav"], **oracle_params(prm))
            c["logs"][kind, which] = (log_from_report(rep, state, **prm), None)
        else:
            c["logs"][kind, which] = tuple(replay(NavBiasStages(O, c["seq"], c["P"], c["G"], *c["starts"]["navb"], cholesky=ch), **prm)
                                           for ch in (False, True))
    return c["logs"][kind, which]


def inertial_floor(O, which):
    """The noise floor of the inertial cases: measured on the per-keyframe-bias pair, and used for the shared-bias graph
    too, which has one reference only: the same sequence, start, stereo factors, IMU and DVL data and step sizes, and a
    camera system that differs by the 6-wide bias border alone."""
    return value_differences(*inertial_logs(O, "navb", which))


# -- the GPU side: what the recorder of test_lm_branches_gpu.py keeps, compared with a log --------------------------------
def tolerance(floor):
    """{"lin0", "scalars", "state"} tolerances (the classes of value_differences()) of the GPU against the reference log:
    100 x the summation-order sensitivity measured between two CPU references (the GPU sums in a third order, with f64
    atomics in the back-substitution), never tighter than the 1e-11 (kernels) / 1e-8 (after a solve) of the stage tests of
    test_ba_gpu.py."""
    return {"lin0": max(100.0 * floor["lin0"], 1e-11), "scalars": max(100.0 * floor["scalars"], 1e-8),
            "state": max(100.0 * floor["state"], 1e-8)}
