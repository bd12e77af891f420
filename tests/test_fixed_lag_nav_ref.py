"""The numpy statement of the inertial fixed-lag prior (fixed_lag_nav_ref.py) against itself: finite differences of its own
error, the system and the linear error, the order of elimination on a real inertial graph, and the padding rows of a
marginal.  No GPU."""
import numpy as np

import fixed_lag_nav_ref as fn
import fixed_lag_ref as fl
import nav_bias_ref as nbr
from visual_underwater_slam_amd import synth

WALK = (2e-3, 2e-4)


def _state(oracle, rng, n):
    s = synth.nav_sequence(n, 40, 20, bias_walk_sigma=WALK)
    poses = np.stack([oracle.pose_retract(T, np.r_[0.1 * rng.uniform(-1, 1, 3), 0.2 * rng.normal(size=3)]) for T in s["poses_gt"]])
    return s, poses, s["vels_gt"] + 0.05 * rng.normal(size=(n, 3)), 0.01 * rng.normal(size=(n, 6))


def test_error_is_its_quadratic_along_a_ray_from_the_linearisation_point(oracle):
    """Local(x0, x0 Exp(t v)) = t v exactly and velocities and biases move by plain addition, so along such a ray
    error = c + t g^T v + 0.5 t^2 v^T H v: central differences of the error give g^T v and v^T H v to round-off."""
    rng = np.random.default_rng(0)
    n, first, m = 6, 2, 3
    s, _, _, _ = _state(oracle, rng, n)
    W = fn.random_prior(rng, first, s["poses_gt"][first:first + m], s["vels_gt"][first:first + m], s["biases_gt"][first:first + m])
    for _ in range(3):
        v = rng.normal(size=15 * m)

        def at(t):
            poses, vels, biases = s["poses_gt"].copy(), s["vels_gt"].copy(), s["biases_gt"].copy()
            for i in range(m):
                poses[first + i] = oracle.pose_retract(W.x0[i], t * v[15 * i:15 * i + 6])
                vels[first + i] = W.v0[i] + t * v[15 * i + 6:15 * i + 9]
                biases[first + i] = W.b0[i] + t * v[15 * i + 9:15 * i + 15]
            return fn.error(oracle, W, poses, vels, biases)
        h = 1e-3
        e0, ep, em = at(0.0), at(h), at(-h)
        assert abs(e0 - W.c) < 1e-14
        assert abs((ep - em) / (2 * h) - W.g @ v) < 1e-9 * max(1.0, abs(W.g @ v))
        assert abs((ep - 2 * e0 + em) / h ** 2 - v @ W.H @ v) < 1e-6 * (v @ W.H @ v)


def test_system_and_linear_error_agree_with_the_error(oracle):
    rng = np.random.default_rng(1)
    n, first, m = 7, 3, 4
    s, poses, vels, biases = _state(oracle, rng, n)
    W = fn.random_prior(rng, first, s["poses_gt"][first:first + m], s["vels_gt"][first:first + m], s["biases_gt"][first:first + m])
    H, g, e = fn.system(oracle, W, poses, vels, biases, n)
    assert e == fn.error(oracle, W, poses, vels, biases)
    d = fn.delta(oracle, W, poses, vels, biases).reshape(m, 15)
    assert min(np.abs(d[:, :6]).max(), np.abs(d[:, 6:9]).max(), np.abs(d[:, 9:]).max()) > 1e-3       # all three kinds
    assert np.array_equal(d[:, 6:9], vels[first:first + m] - W.v0) and np.array_equal(d[:, 9:], biases[first:first + m] - W.b0)
    r = fn.rows(first, m)
    assert len(r) == 15 * m and np.array_equal(H[np.ix_(r, r)], W.H) and np.array_equal(g[r], W.g + W.H @ d.reshape(-1))
    out = np.ones(18 * n, bool)
    out[r] = False                                                    # the other keyframes AND this window's padding
    assert out[fn.pad_rows(first, m)].all() and not H[out].any() and not H[:, out].any() and not g[out].any()
    x = 0.01 * rng.normal(size=18 * n)
    u = d.reshape(-1) + x[r]
    want = W.c + W.g @ u + 0.5 * u @ W.H @ u
    assert abs(fn.linear_error(oracle, W, poses, vels, biases, x) - want) < 1e-12 * abs(want)


def test_the_order_of_elimination_and_the_padding_of_a_marginal(oracle):
    """The reduced camera system of a real inertial graph (nav_bias_ref.dense_system at lambda = 0): all dropped keyframes
    at once against node by node with another solver agree to round-off, the padding rows of the marginal are identity rows
    with a zero gradient, and compaction commutes with eliminating the padding as variables."""
    rng = np.random.default_rng(2)
    n, k = 6, 2
    s, poses, vels, biases = _state(oracle, rng, n)
    P, G = nbr.make_graph(oracle, s)
    ref = nbr.dense_system(oracle, s, P, G, poses, vels, biases, s["points_init"], 0.0)
    A, b = ref["A"], ref["g"]
    H, g, c, dev = fn.marginal_head(A, b, ref["err"], k)
    H2, g2, c2, dev2 = fn.marginal_head(A, b, ref["err"], k, one_at_a_time=True, solve="lu")
    assert dev == 0.0 and dev2 < 1e-15
    assert H.shape == (15 * (n - k),) * 2
    scale = np.abs(H).max()
    assert np.abs(H - H2).max() < 1e-9 * scale and np.abs(g - g2).max() < 1e-9 * np.abs(g).max() and abs(c - c2) < 1e-9 * abs(c)
    # the padding eliminated as variables: the same H and g (a unit diagonal with a zero gradient costs nothing)
    elim = list(range(18 * k)) + list(fn.pad_rows(k, n - k))
    H3, g3, c3 = fl.marginal(A, b, ref["err"], elim)
    assert np.abs(H - H3).max() < 1e-9 * scale and np.abs(g - g3).max() < 1e-9 * np.abs(g).max() and abs(c - c3) < 1e-9 * abs(c)


def test_the_reference_smoother_follows_the_dense_batch_on_the_end_to_end_scene(oracle):
    """The scene tests/test_fixed_lag_nav_gpu.py rests its one-sigma bound on, cleared on the CPU first: a dense Gauss-Newton
    fixed-lag smoother with the smoother's own absorbed-set rule ends within one sigma of the dense batch optimum's
    marginal on the newest position."""
    s = fn.smoother_scene()
    n, lag = fn.SMOOTHER["n"], fn.SMOOTHER["lag"]
    bp, _, _, cov = fn.batch_optimum(oracle, s)
    at = 18 * (n - 1) + 3
    one_sigma = float(np.sqrt(np.trace(cov[at:at + 3, at:at + 3])))
    poses, vels, biases, lo, counts = fn.reference_smoother(oracle, s)
    assert lo == n - 1 - lag                               # the last window holds lag + 1 keyframes
    assert [c[0] for c in counts] == [0] * (lag + 1) + [1] * (n - lag - 1)
    assert sum(c[1] for c in counts) > 0 and sum(c[2] for c in counts) > 0      # landmarks marginalised, factors discarded
    diff = float(np.linalg.norm(poses[n - 1, 9:] - bp[n - 1, 9:]))
    print(f"reference smoother against the dense batch: {diff:.4e} m = {diff / one_sigma:.3f} sigma (one sigma {one_sigma:.4e} m)")
    assert diff <= one_sigma
    # and the batch optimum explains the truth: within three sigma on that position
    assert np.linalg.norm(bp[n - 1, 9:] - s["poses_gt"][n - 1, 9:]) <= 3.0 * one_sigma
