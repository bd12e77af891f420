"""The numpy statement of the long-closure path (tests/closure_ref.py) against the dense references of between_ref.py, and
the certification of the LM graphs the GPU tests walk: every decision at least 1e-3 (relative) from its threshold, as
tests/test_lm_branches.py asks of its logs, for the dense loop and for the loop that solves with the low-rank term."""
import numpy as np
import pytest

import between_ref as br
import closure_ref as cr
import lm_ref

MARGIN = 1e-3
_logs = {}


def logs(oracle, name):
    """(dense log, low-rank log) of one LM case, computed once"""
    if name not in _logs:
        truth, init, G, priors = cr.lm_case(name)
        _logs[name] = tuple(lm_ref.replay(cr.PoseGraphStages(oracle, G, priors, init, max_span=m), **cr.LM_CASES[name]["params"])
                            for m in (None, cr.LM_MAX_SPAN))
    return _logs[name]


def test_the_long_sets_blocks_are_u_ut(oracle):
    rng = np.random.default_rng(3)
    truth, init, G, _ = br.pose_graph(rng, 30, closures=[(0, 29), (25, 4), (4, 25), (4, 17)], noise=0.02,
                                      loss=(2, 0.5))
    for stride in (1, 2, 3):
        Gin, Glong = cr.split(G, 5)
        assert len(Glong.i) == 4 and len(Gin.i) == 29
        H, g, e, fac = br.system(oracle, Glong, init, stride * 30, stride)
        U = cr.u_matrix(fac, stride * 30, stride)
        assert np.abs(U @ U.T - H).max() <= 1e-12 * np.abs(H).max()
        R = cr.rows(fac)
        assert R.shape == (4, 78)
        assert np.allclose(U @ R[:, 72:].reshape(-1), g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
        assert abs(0.5 * (R[:, 72:] ** 2).sum() - e) <= 1e-12 * e


def test_lowrank_solve_equals_the_dense_solve(oracle):
    rng = np.random.default_rng(4)
    truth, init, G, priors = br.pose_graph(rng, 40, closures=[(0, 39), (30, 3), (3, 30)], noise=0.01)
    Gin, Glong = cr.split(G, 8)
    A0, g0, _ = br.prior_system(oracle, priors, init)
    Hin, gin, _, _ = br.system(oracle, Gin, init, 40)
    Hl, gl, _, fac = br.system(oracle, Glong, init, 40)
    B = A0 + 1e-3 * np.eye(240) + Hin
    b = -(g0 + gin + gl)
    x = cr.lowrank_solve(B, cr.u_matrix(fac, 40), b)
    ref = np.linalg.solve(B + Hl, b)
    assert np.abs(x - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("name", list(cr.LM_CASES))
def test_lm_cases_are_certified(oracle, name):
    dense, low = logs(oracle, name)
    truth, init, G, priors = cr.lm_case(name)
    if cr.LM_CASES[name]["n"] <= 40:        # the dense replay IS between_ref.lm_optimize
        _, _, rep = br.lm_optimize(oracle, G, init, priors=priors, **lm_ref.oracle_params(cr.LM_CASES[name]["params"]))
        lm_ref.same_report(dense, rep, err_rtol=1e-12)
    seq = "".join(o for _, o, _ in lm_ref.outcomes(dense))
    assert lm_ref.outcomes(dense) == lm_ref.outcomes(low)
    assert dense["lambda_hist"] == low["lambda_hist"]
    floor = lm_ref.value_differences(dense, low)
    for log in (dense, low):
        margin, what = lm_ref.narrowest_margin(log)
        print(f"{name}: trials {seq}, narrowest margin {margin:.3g} ({what}); floor dense vs low-rank {floor}")
        assert margin >= MARGIN, (margin, what)
    if "rough" in cr.LM_CASES[name]:
        assert "R" in seq
    assert len(cr.split(G, cr.LM_MAX_SPAN)[1].i) == len(cr.LM_CASES[name]["closures"]) + ("false" in cr.LM_CASES[name])
