"""The Levenberg-Marquardt loop away from the starts where Gauss-Newton already works: rejected trials, the lambda bounds
and factor, the model-fidelity threshold, stop_search, every stop rule and the two early returns -- on the CPU, between the
references alone.  For every case of lm_ref.STEREO_CASES the replay of lm_ref.py over the scalar oracle's stage functions
must tell what oracle.ba_lm_optimize and BAPort.optimize tell, reach the outcome the table lists, and take every decision
far from its threshold, so that test_lm_branches_gpu.py may demand the same decisions of the GPU exactly.  The family
cases of lm_ref.family_case() are checked the same way against each family's own LM."""
import numpy as np
import pytest

import lm_ref

MARGIN = 1e-3       # every compared quantity of a reference log is at least this far, relatively, from its threshold


@pytest.mark.parametrize("name", list(lm_ref.STEREO_CASES))
def test_replay_equals_the_c_oracle_and_the_port(oracle, name):
    """outer, tries, iterations, status, lambda_hist and final lambda exactly; err_hist exactly against the C loop (the same
    stage functions in the same order), within the solve tolerance 1e-8 against BAPort (other kernels, LAPACK)"""
    sc = lm_ref.stereo_scene(oracle)
    start, prm, _ = lm_ref.STEREO_CASES[name]
    po, pt = sc["starts"][start]
    log, plog, port = lm_ref.stereo_logs(oracle, name)
    oposes, opoints, orep = oracle.ba_lm_optimize(sc["P"], sc["band"], po, pt, **lm_ref.oracle_params(prm))
    lm_ref.same_report(log, orep)
    assert log["initial_error"] == orep["initial_error"]
    assert np.array_equal(log["state"][0], oposes) and np.array_equal(log["state"][1], opoints)
    pposes, ppoints, prep = port.optimize(po, pt, **lm_ref.oracle_params(prm))
    lm_ref.same_report(log, prep, 1e-8)
    lm_ref.same_report(plog, prep, 1e-8)
    assert lm_ref.outcomes(log) == lm_ref.outcomes(plog)
    assert lm_ref.relerr(pposes, oposes) <= 1e-8 and lm_ref.relerr(ppoints, opoints) <= 1e-8


@pytest.mark.parametrize("name", list(lm_ref.STEREO_CASES))
def test_reference_outcome_and_wide_margins(oracle, name):
    """the outcome the table lists, and no decision within MARGIN of its threshold; prints the case's noise floor: the
    largest relative difference between the two references in lin0, in lin1 / new1 and in the trial states"""
    start, prm, (tries, outer, accepted, status, lam_hist) = lm_ref.STEREO_CASES[name]
    log, plog, _ = lm_ref.stereo_logs(oracle, name)
    seq = "".join(o for _, o, _ in lm_ref.outcomes(log))
    margin, what = lm_ref.narrowest_margin(log)
    floor = lm_ref.value_differences(log, plog)
    tol = lm_ref.tolerance(floor)
    print(f"{name}: {start} {prm}: trials {seq}, lambda_hist {log['lambda_hist']}, err_hist {log['err_hist']}; narrowest margin "
          f"{margin:.3g} ({what}); noise floor lin0 {floor['lin0']:.2g} scalars {floor['scalars']:.2g} state {floor['state']:.2g} "
          f"-> tolerance {tol['lin0']:.2g} / {tol['scalars']:.2g} / {tol['state']:.2g}")
    assert (log["tries"], log["outer"], log["iterations"], log["status"]) == (tries, outer, accepted, status)
    assert log["tries"] <= 25
    if lam_hist is not None:
        assert np.allclose(log["lambda_hist"], lam_hist, rtol=1e-12, atol=0)
    assert margin >= MARGIN, (margin, what)
    assert all(t["status"] == 0 for t in log["trials"])
    if not tries:               # an early return: nothing ran and the state is the start, bit for bit
        sc = lm_ref.stereo_scene(oracle)
        assert all(np.array_equal(a, b) for a, b in zip(log["state"], sc["starts"][start]))


def test_named_outcomes_of_the_table(oracle):
    """what the rows are there for: the lambda schedules, the clamp that binds and the one that does not, and the stops"""
    L = {name: lm_ref.stereo_logs(oracle, name)[0] for name in lm_ref.STEREO_CASES}
    d = L["defaults"]
    assert [round(t["lam"], 12) for t in d["trials"][:9]] == [round(1e-5 * 10.0 ** k, 12) for k in range(9)]
    assert np.allclose(d["err_hist"], [187690.048, 115131.183, 83328.284], rtol=1e-8)
    assert [round(t["fidelity"], 2) for t in d["trials"][-5:]] == [0.53, -5.34, 0.78, -1976.41, 1.61]
    assert L["upper-bound"]["final_lambda"] == pytest.approx(0.01, rel=1e-12)
    s = L["stop-search"]
    assert s["trials"][-1]["outcome"] == "S" and not s["trials"][-1]["accepted"] and s["trials"][-1]["fidelity"] < 0.9
    f3 = L["factor-3"]["lambda_hist"]
    assert np.allclose(f3, [1e-5 * 3.0 ** 16, 1e-5 * 3.0 ** 15, 1e-5 * 3.0 ** 15], rtol=1e-12)
    assert min(L["lower-bound-free"]["lambda_hist"]) > 10.0 and L["lower-bound-binds"]["lambda_hist"][1:] == [10.0] * 5
    for name in ("error-tol", "absolute-tol"):
        assert L[name]["outers"][-1]["converged"] and not L[name]["outers"][0]["converged"]
    assert L["error-tol"]["final_error"] <= 1e3 and L["absolute-tol"]["outers"][-1]["abs_dec"] <= 1e4
    assert L["absolute-tol"]["outers"][-1]["rel_dec"] > 1e-5          # the absolute tolerance alone stops it


def test_both_ends_of_a_search_occur(oracle):
    """over the table: a step accepted after at least one rejection, and a search abandoned (by stop_search and by the upper
    bound) after at least one rejection"""
    seen = set()
    for name in lm_ref.STEREO_CASES:
        log = lm_ref.stereo_logs(oracle, name)[0]
        for k in range(log["outer"]):
            group = "".join(t["outcome"] for t in log["trials"] if t["outer"] == k)
            if len(group) > 1:
                seen.add(group[-1])
    assert seen == {"A", "S", "U"}, seen


# -- the C loops return their trials ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["defaults", "stop-search", "fidelity-0.9", "lower-bound-binds"])
def test_the_c_oracle_reports_the_trials_of_the_replay(oracle, name):
    """lambda, lin0, lin1, new1 and the status of every linear solve in oracle.ba_lm_optimize's report: the replay's, bit for
    bit, and the same decisions read back from them"""
    sc = lm_ref.stereo_scene(oracle)
    start, prm, _ = lm_ref.STEREO_CASES[name]
    log = lm_ref.stereo_logs(oracle, name)[0]
    *state, rep = oracle.ba_lm_optimize(sc["P"], sc["band"], *sc["starts"][start], **lm_ref.oracle_params(prm))
    assert rep["trials"] == [(t["lam"], t["lin0"], t["lin1"], t["new1"], t["status"]) for t in log["trials"]]
    clog = lm_ref.log_from_report(rep, state, **prm)
    assert lm_ref.outcomes(clog) == lm_ref.outcomes(log)
    assert [t["fidelity"] for t in clog["trials"]] == [t["fidelity"] for t in log["trials"]]
    assert lm_ref.narrowest_margin(clog) == lm_ref.narrowest_margin(log)


# -- the other configurations: each rejects from its rough start, with every decision wide --------------------------------
def _rough(log, what):
    seq = "".join(o for _, o, _ in lm_ref.outcomes(log))
    margin, where = lm_ref.narrowest_margin(log)
    print(f"{what}: trials {seq}, status {log['status']}, lambda_hist {log['lambda_hist']}, err_hist {log['err_hist']}; narrowest "
          f"margin {margin:.3g} ({where})")
    assert "R" in seq and log["tries"] <= 25 and margin >= MARGIN, (seq, margin, where)
    assert all(t["status"] == 0 for t in log["trials"])
    return seq


def _floor(log, twin):
    """the pair takes the same decisions; prints the noise floor measured on it and the tolerance that follows"""
    assert lm_ref.outcomes(log) == lm_ref.outcomes(twin)
    floor = lm_ref.value_differences(log, twin)
    tol = lm_ref.tolerance(floor)
    print(f"   noise floor lin0 {floor['lin0']:.2g} scalars {floor['scalars']:.2g} state {floor['state']:.2g} -> tolerance "
          f"{tol['lin0']:.2g} / {tol['scalars']:.2g} / {tol['state']:.2g}")


@pytest.mark.parametrize("which", list(lm_ref.FAMILY_PARAMS))
@pytest.mark.parametrize("name", list(lm_ref.FAMILIES))
def test_stereo_configurations_reject_from_their_start(oracle, name, which):
    """robust, extrinsic, mono, and between factors + landmark priors + pose fixes: the replay tells what the family's own
    RobustBA.lm tells, bit for bit (the same stages in the same order)"""
    c = lm_ref.family_case(oracle, name)
    log, twin = lm_ref.family_logs(oracle, name, which)
    seq = _rough(log, f"{name} {which}")
    _floor(log, twin)
    assert log["status"] == (1 if which == "defaults" else 2) and ("A" in seq) == (which == "defaults" or name == "cauchy")
    poses, points, rep = c["R"].lm(*c["start"], **lm_ref.FAMILY_PARAMS[which])
    lm_ref.same_report(log, rep)
    assert np.array_equal(poses, log["state"][0]) and np.array_equal(points, log["state"][1])


def test_between_terms_in_the_composed_reference_equal_between_ref_lm(oracle):
    """lm_ref.BetweenFixesBA adds between_ref's factors to the RobustBA solve; on stereo + between factors alone (no landmark
    priors, no fixes) its replay walks between_ref.lm_optimize's trials: the same (lambda, accepted) sequence, err_hist to
    the solve tolerance (dense solve of the whole system there, Cholesky of the reduced one here)"""
    import between_ref
    c = lm_ref.family_case(oracle, "between+priors+fixes")
    seq, R = c["seq"], c["R"]
    plain = lm_ref.between_fixes_ba(oracle, dict(n_poses=R.nP, n_points=R.nL, n_obs=R.nO, obs_pose=R.op, obs_point=R.ol, meas=R.meas),
                                    seq["K"], seq["sigma"], 0, 0.0, None, np.zeros(R.nO, bool), seq["mono_K"], seq["mono_sigma"],
                                    (np.array([0]), seq["poses_gt"][:1], seq["prior_sigmas"][None]), between=c["between"])
    prm = dict(maxIterations=3)
    log = lm_ref.replay(lm_ref.RobustStages(plain, *c["start"]), **prm)
    _rough(log, "stereo + between")
    import torch
    from visual_underwater_slam_amd import ba_pack
    pk = ba_pack.pack_observations(torch.from_numpy(seq["obs_pose"]), torch.from_numpy(seq["obs_point"]), torch.from_numpy(seq["meas"]),
                                   R.nP, R.nL)
    P = oracle.BAProblem(pk, seq["K"], seq["sigma"], (np.array([0], np.int32), seq["poses_gt"][:1], seq["prior_sigmas"][None]))
    band = max(ba_pack.build_structure(pk)["band"], c["between"].span)
    poses, points, rep = between_ref.lm_optimize(oracle, c["between"], c["start"][0], P=P, points=c["start"][1], band=band,
                                                 **lm_ref.oracle_params(prm))
    assert rep["trials"] == [(t["lam"], t["accepted"]) for t in log["trials"]]
    lm_ref.same_report(log, rep, 1e-8)
    assert lm_ref.relerr(poses, log["state"][0]) <= 1e-8 and lm_ref.relerr(points, log["state"][1]) <= 1e-8


@pytest.mark.parametrize("which", list(lm_ref.FAMILY_PARAMS))
def test_split_scene_rejects_from_its_start(oracle, which):
    """the 72-keyframe line: scalar oracle and BAPort take the same decisions; prints the noise floor of the pair"""
    log, plog = lm_ref.split_logs(oracle, which)
    _rough(log, f"split {which}")
    _floor(log, plog)


@pytest.mark.parametrize("which", list(lm_ref.FAMILY_PARAMS))
@pytest.mark.parametrize("kind", ["nav", "navb"])
def test_inertial_layouts_reject_from_their_start(oracle, kind, which):
    """shared bias: the log read from oracle.nav_lm_optimize's trials; one bias per keyframe: the replay over
    nav_bias_ref.lm_trial tells what nav_bias_ref.lm_optimize tells, bit for bit"""
    import nav_bias_ref
    log, twin = lm_ref.inertial_logs(oracle, kind, which)
    _rough(log, f"{kind} {which}")
    if twin is not None:
        _floor(log, twin)
    assert log["status"] == (1 if which == "defaults" else 2)
    if kind == "navb":
        c = lm_ref.inertial_case(oracle)
        *state, rep = nav_bias_ref.lm_optimize(oracle, c["seq"], c["P"], c["G"], *c["starts"]["navb"],
                                               **lm_ref.oracle_params(lm_ref.FAMILY_PARAMS[which]))
        lm_ref.same_report(log, rep)
        assert rep["trials"] == [(t["lam"], t["accepted"]) for t in log["trials"]]
        assert all(np.array_equal(a, b) for a, b in zip(state, log["state"]))
