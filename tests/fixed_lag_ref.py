"""numpy f64 statement of fixed-lag smoothing (include/vus_fixed_lag.h): the dense prior over a window of consecutive poses
-- error, gradient, dense system, linear error at a step -- and the marginal (H, g, c) a graph leaves on its kept variables,
by the Schur complement of a dense full Hessian over poses AND landmarks.  Test infrastructure only (a plain module)."""
from collections import namedtuple

import numpy as np

from marginals_ref import sym3

# first pose, x0 [m, 12], H [6m, 6m], g [6m], c
Prior = namedtuple("Prior", "first x0 H g c")


def delta(oracle, W, poses):
    """The stack of Local(x0_i, x_{first + i}), 6 m values."""
    return np.concatenate([oracle.pose_local(W.x0[i], poses[W.first + i]) for i in range(len(W.x0))])


def error(oracle, W, poses):
    """c + g^T d + 0.5 d^T H d."""
    d = delta(oracle, W, poses)
    return float(W.c + W.g @ d + 0.5 * d @ W.H @ d)


def system(oracle, W, poses, n_poses):
    """The prior linearised at poses over all n_poses poses: (H [6n, 6n], gradient g + H d [6n], error(poses)).  The
    derivative of Local is not applied."""
    d = delta(oracle, W, poses)
    m = len(W.x0)
    s = slice(6 * W.first, 6 * (W.first + m))
    H, g = np.zeros((6 * n_poses, 6 * n_poses)), np.zeros(6 * n_poses)
    H[s, s] = W.H
    g[s] = W.g + W.H @ d
    return H, g, float(W.c + W.g @ d + 0.5 * d @ W.H @ d)


def linear_error(oracle, W, poses, x):
    """error(poses) + (g + H d)^T dx + 0.5 dx^T H dx at the node step x [6 n_poses]."""
    H, g, e = system(oracle, W, poses, len(x) // 6)
    return float(e + g @ x + 0.5 * x @ H @ x)


def marginal(A, b, e0, elim, solve="cholesky"):
    """The quadratic e0 + b^T y + 0.5 y^T A y minimised over the variables `elim` (scalar indices): (H, g, c) on the rest,
    in ascending order.  H = A_KK - A_KE A_EE^-1 A_EK, g = b_K - A_KE A_EE^-1 b_E, c = e0 - 0.5 b_E^T A_EE^-1 b_E.
    `solve`: "cholesky" (A_EE = L L^T, two triangular solves) or "lu" (np.linalg.solve) -- two orders of the same sums."""
    n = len(b)
    E = np.asarray(sorted(elim), dtype=np.int64)
    K = np.setdiff1d(np.arange(n), E)
    AEE, AKE, rhs = A[np.ix_(E, E)], A[np.ix_(K, E)], np.column_stack([A[np.ix_(E, K)], b[E]])
    if solve == "cholesky":
        L = np.linalg.cholesky(AEE)
        X = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    else:
        X = np.linalg.solve(AEE, rhs)
    H = A[np.ix_(K, K)] - AKE @ X[:, :-1]
    return 0.5 * (H + H.T), b[K] - AKE @ X[:, -1], float(e0 - 0.5 * b[E] @ X[:, -1])


def marginal_head(A, b, e0, n_drop, one_at_a_time=False, solve="cholesky"):
    """marginal() over the first n_drop 6-blocks; `one_at_a_time` eliminates them node by node (the same result in another
    order of operations)."""
    if not one_at_a_time:
        return marginal(A, b, e0, range(6 * n_drop), solve)
    for _ in range(n_drop):
        A, b, e0 = marginal(A, b, e0, range(6), solve)
    return A, b, e0


def full_dense(lin, obs_pose, obs_point, n_poses, n_points):
    """The dense Hessian and gradient over [poses (6 each), landmarks (3 each)] from the products of a stereo linearisation
    (Hpp [n_poses, 36], gp, W [n_obs, 18] = the 6 x 3 pose-landmark block of each observation, V [n_points, 6] upper
    triangle, gl) with the observations' pose and landmark indices in the same (landmark-sorted) order."""
    n = 6 * n_poses + 3 * n_points
    A, b = np.zeros((n, n)), np.zeros(n)
    for i in range(n_poses):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = lin["Hpp"][i].reshape(6, 6)
        b[6 * i:6 * i + 6] = lin["gp"][i]
    for j in range(n_points):
        o = 6 * n_poses + 3 * j
        A[o:o + 3, o:o + 3] = sym3(lin["V"][j])
        b[o:o + 3] = lin["gl"][j]
    for k in range(len(obs_pose)):
        i, o = int(obs_pose[k]), 6 * n_poses + 3 * int(obs_point[k])
        w = lin["W"][k].reshape(6, 3)
        A[6 * i:6 * i + 6, o:o + 3] += w
        A[o:o + 3, 6 * i:6 * i + 6] += w.T
    return A, b


def add_poses(A, b, H, g):
    """A, b over [poses, landmarks] plus a pose-side system H [6n, 6n], g (between factors, a window prior)."""
    A, b = A.copy(), b.copy()
    n = len(g)
    A[:n, :n] += H
    b[:n] += g
    return A, b
