"""The numpy statement of fixed-lag smoothing (fixed_lag_ref.py) against itself: finite differences of its own error, the
order of elimination, and the constant as the minimum of the linearised cost.  No GPU."""
import numpy as np

import between_ref as br
import fixed_lag_ref as fl
import marginals_ref as mr


def _prior(rng, oracle, n, first, m, psd_rank=None):
    truth, init, _, _ = br.pose_graph(rng, n)
    M = rng.normal(size=(6 * m, psd_rank or 6 * m))
    H = M @ M.T
    return truth, init, fl.Prior(first, truth[first:first + m].copy(), H, rng.normal(size=6 * m), 0.7)


def test_error_is_its_quadratic_along_a_retraction_of_x0(oracle):
    """Local(x0, x0 Exp(t v)) = t v exactly, so along such a ray error = c + t g^T v + 0.5 t^2 v^T H v: central differences
    of the error give g^T v and v^T H v to round-off."""
    rng = np.random.default_rng(0)
    n, first, m = 7, 2, 3
    _, _, W = _prior(rng, oracle, n, first, m)
    for _ in range(4):
        v = rng.normal(size=6 * m)

        def at(t):
            poses = np.tile(W.x0[0], (n, 1))
            for i in range(m):
                poses[first + i] = oracle.pose_retract(W.x0[i], t * v[6 * i:6 * i + 6])
            return fl.error(oracle, W, poses)
        h = 1e-3
        e0, ep, em = at(0.0), at(h), at(-h)
        assert abs(e0 - W.c) < 1e-14
        assert abs((ep - em) / (2 * h) - W.g @ v) < 1e-9 * max(1.0, abs(W.g @ v))
        assert abs((ep - 2 * e0 + em) / h ** 2 - v @ W.H @ v) < 1e-6 * (v @ W.H @ v)


def test_system_and_linear_error_agree_with_the_error(oracle):
    """Away from x0: the system's error is error(x), its gradient g + H delta sits in the window's rows, and the linear
    error at a step is the quadratic model -- which is the true error of x0-side steps, error being quadratic in delta."""
    rng = np.random.default_rng(1)
    n, first, m = 9, 4, 5
    _, init, W = _prior(rng, oracle, n, first, m)
    H, g, e = fl.system(oracle, W, init, n)
    assert e == fl.error(oracle, W, init)
    d = fl.delta(oracle, W, init)
    assert np.abs(d).max() > 1e-3                                    # delta != 0
    s = slice(6 * first, 6 * (first + m))
    assert np.array_equal(H[s, s], W.H) and np.allclose(g[s], W.g + W.H @ d, rtol=0, atol=0)
    out = np.ones(6 * n, bool)
    out[s] = False
    assert not H[out].any() and not H[:, out].any() and not g[out].any()
    x = 0.01 * rng.normal(size=6 * n)
    want = W.c + W.g @ (d + x[s]) + 0.5 * (d + x[s]) @ W.H @ (d + x[s])
    assert abs(fl.linear_error(oracle, W, init, x) - want) < 1e-12 * abs(want)
    # finite differences of the linear error in the step: gradient g + H delta, curvature H
    v = rng.normal(size=6 * n)
    h = 1e-3
    lp, lm, l0 = (fl.linear_error(oracle, W, init, t * v) for t in (h, -h, 0.0))
    assert abs((lp - lm) / (2 * h) - g @ v) < 1e-8 * max(1.0, abs(g @ v))
    assert abs((lp - 2 * l0 + lm) / h ** 2 - v @ H @ v) < 1e-6 * (v @ H @ v)


def test_two_nodes_at_once_is_one_node_twice():
    rng = np.random.default_rng(2)
    A, _ = mr.random_spd_band(rng, 9, 4)
    b, e0 = rng.normal(size=54), 3.0
    H2, g2, c2 = fl.marginal_head(A, b, e0, 2)
    H1, g1, c1 = fl.marginal_head(A, b, e0, 2, one_at_a_time=True)
    scale = np.abs(H2).max()
    assert np.abs(H1 - H2).max() < 1e-13 * scale and np.abs(g1 - g2).max() < 1e-13 * np.abs(g2).max() and abs(c1 - c2) < 1e-13
    Hl, gl, cl = fl.marginal_head(A, b, e0, 2, solve="lu")
    assert np.abs(Hl - H2).max() < 1e-13 * scale and np.abs(gl - g2).max() < 1e-13 * np.abs(g2).max() and abs(cl - c2) < 1e-13


def test_the_constant_is_the_minimum_of_the_linearised_cost():
    """c = min over the eliminated variables of the quadratic at a zero step of the kept ones, and the reduced quadratic at
    any kept step is the minimum of the full one over the eliminated variables -- by a dense solve."""
    rng = np.random.default_rng(3)
    n = 40
    M = rng.normal(size=(n, n))
    A, b, e0 = M @ M.T + n * np.eye(n), rng.normal(size=n), 1.5
    elim = [0, 1, 2, 3, 4, 5, 17, 18, 19, 33]
    keep = np.setdiff1d(np.arange(n), elim)
    H, g, c = fl.marginal(A, b, e0, elim)

    def full(y):
        return e0 + b @ y + 0.5 * y @ A @ y
    for xk in (np.zeros(len(keep)), rng.normal(size=len(keep))):
        y = np.zeros(n)
        y[keep] = xk
        y[elim] = np.linalg.solve(A[np.ix_(elim, elim)], -(b[elim] + A[np.ix_(elim, keep)] @ xk))
        want = full(y)
        got = c + g @ xk + 0.5 * xk @ H @ xk
        assert abs(got - want) < 1e-12 * max(1.0, abs(want))
        for _ in range(3):                                         # a minimum: any other choice costs more
            y2 = y.copy()
            y2[elim] += 0.1 * rng.normal(size=len(elim))
            assert full(y2) > want
