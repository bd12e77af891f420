"""numpy f64 statement of the fixed-lag prior of an inertial window (include/vus_fixed_lag_nav.h): the dense prior over pose,
velocity and bias of consecutive keyframes -- delta, error, dense system over the nodes of the per-keyframe-bias layout,
linear error at a step -- the 18 -> 15 compaction of a marginal, and the dense graph [nodes, landmarks] such a marginal is
taken from.  It sits on nav_bias_ref.py (the inertial factors) and fixed_lag_ref.py (marginal / marginal_head).  Test
infrastructure only (a plain module)."""
from collections import namedtuple

import numpy as np

import fixed_lag_ref as fl
import nav_bias_ref as nbr

# first keyframe, x0 [m, 12], v0 [m, 3], b0 [m, 6], H [15m, 15m], g [15m], c
NavPrior = namedtuple("NavPrior", "first x0 v0 b0 H g c")

KEEP18 = np.r_[0:9, 12:18]          # the 15 tangent coordinates of a keyframe among its 18 node coordinates
PAD18 = np.r_[9:12]                 # the padding of its velocity node


def rows(first, m):
    """The node coordinates (of 18 per keyframe) of the 15 m tangent coordinates of keyframes first .. first + m - 1."""
    return np.concatenate([18 * (first + i) + KEEP18 for i in range(m)])


def pad_rows(first, m):
    return np.concatenate([18 * (first + i) + PAD18 for i in range(m)])


def delta(oracle, W, poses, vels, biases):
    """Per window keyframe: Local(x0_i, x_i), v_i - v0_i, b_i - b0_i; 15 m values."""
    out = []
    for i in range(len(W.x0)):
        k = W.first + i
        out += [oracle.pose_local(W.x0[i], poses[k]), vels[k] - W.v0[i], biases[k] - W.b0[i]]
    return np.concatenate(out)


def error(oracle, W, poses, vels, biases):
    """c + g^T d + 0.5 d^T H d."""
    d = delta(oracle, W, poses, vels, biases)
    return float(W.c + W.g @ d + 0.5 * d @ W.H @ d)


def system(oracle, W, poses, vels, biases, n):
    """The prior linearised at the state over the 3 n nodes of n keyframes: (H [18n, 18n], gradient g + H d [18n], the error
    there).  The derivative of Local is not applied; the padding coordinates get nothing."""
    d = delta(oracle, W, poses, vels, biases)
    r = rows(W.first, len(W.x0))
    H, g = np.zeros((18 * n, 18 * n)), np.zeros(18 * n)
    H[np.ix_(r, r)] = W.H
    g[r] = W.g + W.H @ d
    return H, g, float(W.c + W.g @ d + 0.5 * d @ W.H @ d)


def linear_error(oracle, W, poses, vels, biases, x):
    """error + (g + H d)^T dx + 0.5 dx^T H dx at the node step x [18 n]."""
    H, g, e = system(oracle, W, poses, vels, biases, len(x) // 18)
    return float(e + g @ x + 0.5 * x @ H @ x)


def compact(H18, g18):
    """A marginal over whole keyframes at 18 coordinates each -> (H [15w, 15w], g [15w], the largest deviation of its padding
    rows and columns from identity rows with a zero gradient)."""
    w = len(g18) // 18
    r, p = rows(0, w), pad_rows(0, w)
    E = H18.copy()
    E[p, p] -= 1.0
    dev = max(np.abs(E[p]).max(), np.abs(E[:, p]).max(), np.abs(g18[p]).max())
    return H18[np.ix_(r, r)], g18[r], float(dev)


def marginal_head(A, b, e0, n_drop, **kw):
    """fixed_lag_ref.marginal_head over the 3 n_drop nodes of the first n_drop keyframes, compacted: (H, g, c, dev)."""
    H18, g18, c = fl.marginal_head(A, b, e0, 3 * n_drop, **kw)
    H, g, dev = compact(H18, g18)
    return H, g, c, dev


def sub_graph(G, kf0, n, imu=None, dvl=None, vp=None, bb=None, bp=None):
    """The BiasGraph of the factors the boolean masks select (None: none of that kind), re-indexed to keyframes kf0 .. of n."""
    pick = lambda mask, k: np.zeros(k, bool) if mask is None else np.asarray(mask, bool)
    mi, md, mv, mb, mp = (pick(imu, len(G.imu_i)), pick(dvl, len(G.dvl_pose)), pick(vp, len(G.vp_idx)), pick(bb, len(G.bb_i)),
                          pick(bp, len(G.bp_idx)))
    out = nbr.BiasGraph(G.g,
                        imu=(G.imu_i[mi] - kf0, G.imu_pim[mi], G.imu_W[mi]) if mi.any() else None,
                        dvl=(G.dvl_pose[md] - kf0, G.dvl_meas[md], 1.0 / G.dvl_w[md]) if md.any() else None,
                        vprior=(G.vp_idx[mv] - kf0, G.vp_v[mv], 1.0 / G.vp_w[mv]) if mv.any() else None,
                        bbetween=(G.bb_i[mb] - kf0, G.bb_meas[mb], 1.0 / G.bb_w[mb]) if mb.any() else None,
                        bprior=(G.bp_idx[mp] - kf0, G.bp_mean[mp], 1.0 / G.bp_w[mp]) if mp.any() else None)
    for idx, reach in ((out.imu_i, 1), (out.dvl_pose, 0), (out.vp_idx, 0), (out.bb_i, 1), (out.bp_idx, 0)):
        assert len(idx) == 0 or (idx.min() >= 0 and idx.max() + reach < n)
    return out


def full_dense(oracle, lin, e_stereo, obs_pose, obs_point, G, poses, vels, biases, n_points, extra=None):
    """Dense (A, b, e0) over [3 n nodes (6 each), landmarks (3 each)] of an inertial graph at (poses, vels, biases): the
    products of a stereo linearisation (fixed_lag_ref.full_dense; `e_stereo` its error, pose priors included) moved to the
    pose nodes, the inertial factors by nav_bias_ref.inertial_system, a unit diagonal on the velocity padding, and an
    optional node-side system `extra` = (H [18n, 18n], g, e), a nav window prior's."""
    n = len(poses)
    As, bs = fl.full_dense(lin, obs_pose, obs_point, n, n_points)
    at = np.concatenate([np.concatenate([18 * i + np.arange(6) for i in range(n)]), 18 * n + np.arange(3 * n_points)])
    N = 18 * n + 3 * n_points
    A, b = np.zeros((N, N)), np.zeros(N)
    A[np.ix_(at, at)] = As
    b[at] = bs
    Hn, gn, en, _ = nbr.inertial_system(oracle, G, poses, vels, biases)
    A[:18 * n, :18 * n] += Hn
    b[:18 * n] += gn
    p = pad_rows(0, n)
    A[p, p] += 1.0
    e0 = e_stereo + en
    if extra is not None:
        A[:18 * n, :18 * n] += extra[0]
        b[:18 * n] += extra[1]
        e0 += extra[2]
    return A, b, float(e0)


def random_prior(rng, first, x0, v0, b0, singular=False):
    """A random positive definite prior on the given linearisation point; `singular`: H v = 0 along one direction."""
    m = len(x0)
    M = rng.normal(size=(15 * m, 15 * m + 3))
    H = M @ M.T
    if singular:
        v = rng.normal(size=15 * m)
        Pm = np.eye(15 * m) - np.outer(v, v) / (v @ v)
        H = Pm @ H @ Pm
    return NavPrior(first, np.array(x0, float), np.array(v0, float), np.array(b0, float), 0.5 * (H + H.T), rng.normal(size=15 * m), 0.37)


# -- the end-to-end scene of the smoother tests ------------------------------------------------------------------------------
WALK = (2e-3, 2e-4)                 # bias random-walk step per keyframe (acc, gyro)
SMOOTHER = dict(n=16, lag=6, stereo_sigma=1.0, dvl_sigma=0.1, vprior_sigma=0.1, bias_prior_sigma=(0.1, 0.01))


def smoother_scene():
    """16 keyframes over about 120 landmarks with a drifting bias; stereo and DVL noise drawn at the sigmas the noise models
    state (SMOOTHER), the bias walk at WALK per keyframe, which is the sigma of the bias between-factors."""
    from visual_underwater_slam_amd import synth
    s = dict(synth.nav_sequence(SMOOTHER["n"], 800, 40, bias_walk_sigma=WALK, meas_sigma=SMOOTHER["stereo_sigma"],
                                dvl_sigma=SMOOTHER["dvl_sigma"]))
    s["sigma"] = SMOOTHER["stereo_sigma"]
    assert len(s["points_gt"]) <= 200
    return s


def landmark_stamp(j, first, latest):
    """The two kinds of landmark timestamp of the smoother tests: the first sighting (even j), the latest sighting (odd j)."""
    return float(latest if j % 2 else first)


def smoother_graph(s):
    """The inertial factors of the smoother scene as a nav_bias_ref.BiasGraph: what tests/test_fixed_lag_nav_gpu.py builds as
    gtsam factors -- ImuFactor and bias walk for every interval, DVL on keyframes 1 .., the priors on V(0) and B(0)."""
    n = len(s["poses_gt"])
    pims, Ws = nbr.preintegrate(s)
    return nbr.BiasGraph(s["gravity"], imu=(np.arange(n - 1), pims, Ws),
                         dvl=(np.arange(1, n), s["dvl"][1:], np.full(n - 1, SMOOTHER["dvl_sigma"])),
                         vprior=(np.array([0]), s["vels_gt"][:1], np.full((1, 3), SMOOTHER["vprior_sigma"])),
                         bbetween=(np.arange(n - 1), np.zeros((n - 1, 6)), np.tile(np.repeat(WALK, 3), (n - 1, 1))),
                         bprior=(np.array([0]), np.zeros((1, 6)), np.repeat(SMOOTHER["bias_prior_sigma"], 3)[None]))


class DenseWindow:
    """A part of the smoother scene as a dense problem: keyframes lo .. hi, the observation rows `rows`, the inertial
    factors between and on those keyframes from `lo_f` on (an absorbed sub-graph takes only those below its `hi_f`), an
    optional NavPrior on its leading keyframes.  At most 16 keyframes and 200 landmarks: everything is dense numpy."""

    def __init__(self, oracle, s, G, lo, hi, rows, prior=None, factors_below=None):
        import torch
        from visual_underwater_slam_amd import ba_pack
        self.o, self.lo, self.n, self.prior = oracle, lo, hi - lo + 1, prior
        rows = np.asarray(sorted(rows), np.int64)
        self.lms = np.unique(s["obs_point"][rows])
        lm_map = -np.ones(len(s["points_gt"]), np.int64)
        lm_map[self.lms] = np.arange(len(self.lms))
        op, ol = s["obs_pose"][rows].astype(np.int64) - lo, lm_map[s["obs_point"][rows]]
        assert self.n <= 16 and len(self.lms) <= 200 and (op >= 0).all() and (op < self.n).all()
        pk = ba_pack.pack_observations(torch.from_numpy(op), torch.from_numpy(ol), torch.from_numpy(s["meas"][rows]), self.n,
                                       len(self.lms))
        pri = (np.array([0], np.int32), s["poses_gt"][:1], s["prior_sigmas"][None]) if lo == 0 else None
        self.P = oracle.BAProblem(pk, s["K"], s["sigma"], pri)
        top = hi + 1 if factors_below is None else factors_below           # factors on keyframes lo <= idx < top
        inside = lambda idx, reach: (idx >= lo) & (idx < top) & (idx + reach <= hi)
        self.G = sub_graph(G, lo, self.n, imu=inside(G.imu_i, 1), dvl=inside(G.dvl_pose, 0), vp=inside(G.vp_idx, 0),
                           bb=inside(G.bb_i, 1), bp=inside(G.bp_idx, 0))

    def system(self, poses, vels, biases, points, lam):
        """The reduced camera system (landmarks eliminated) at the state, the prior included: (A, g, the stereo pieces)."""
        ref = nbr.dense_system(self.o, None, self.P, self.G, poses, vels, biases, points, lam, band=max(self.n - 1, 0))
        A, g = ref["A"].copy(), ref["g"].copy()
        if self.prior is not None:
            Hp, gp, _ = system(self.o, self.prior, poses, vels, biases, self.n)
            A += Hp
            g += gp
        return A, g, ref

    def error(self, poses, vels, biases, points):
        e = nbr.total_error(self.o, self.P, self.G, poses, vels, biases, points)
        return e + (error(self.o, self.prior, poses, vels, biases) if self.prior is not None else 0.0)

    def optimize(self, poses, vels, biases, points, max_iterations=30):
        """Gauss-Newton with Levenberg's damping as the safeguard: a step that does not lower the error is retried at ten
        times the damping.  Returns the state at convergence (relative decrease below 1e-10)."""
        lam, cur = 1e-7, self.error(poses, vels, biases, points)
        for _ in range(max_iterations):
            A, g, ref = self.system(poses, vels, biases, points, lam)
            x = np.linalg.solve(A, -g)
            dp = nbr.split_step(x, self.n)[0]
            dl = self.o.ba_backsub(self.P, ref["lin"], ref["sch"]["Vinv"], dp)
            npo, nv, nb = nbr.retract(self.o, poses, vels, biases, x)
            npt = points + dl
            new = self.error(npo, nv, nb, npt)
            if new < cur:
                done = cur - new <= 1e-10 * cur
                poses, vels, biases, points, cur, lam = npo, nv, nb, npt, new, max(lam / 10.0, 1e-9)
                if done:
                    break
            else:
                lam *= 10.0
                if lam > 1e6:
                    break
        return poses, vels, biases, points

    def marginal(self, poses, vels, biases, points, n_drop):
        """The NavPrior (first = 0) this graph leaves on its keyframes n_drop .. at the state; c is not carried (0)."""
        A, g, _ = self.system(poses, vels, biases, points, 0.0)
        H, gk, _, dev = marginal_head(A, g, 0.0, n_drop)
        assert dev == 0.0
        return NavPrior(0, poses[n_drop:].copy(), vels[n_drop:].copy(), biases[n_drop:].copy(), H, gk, 0.0)


def reference_smoother(oracle, s, lag=None):
    """The fixed-lag smoother of gtsam_unstable.BatchFixedLagSmoother by dense numpy, one keyframe per update, with its
    absorbed-set rule (timestamps: keyframe i at i, landmarks by landmark_stamp).  Returns the estimates of the last window
    (poses, vels, biases [n], valid from its first keyframe on), that keyframe and the counts per update."""
    n, lag = len(s["poses_gt"]), float(SMOOTHER["lag"] if lag is None else lag)
    G = smoother_graph(s)
    poses, vels, biases, points = s["poses_init"].copy(), np.zeros((n, 3)), np.zeros((n, 6)), s["points_init"].copy()
    vels[0] = s["vels_gt"][0]
    lo, prior, live, present, ts, first_seen, counts = 0, None, set(), set(), {}, {}, []
    for i in range(n):
        if i:
            vels[i], biases[i] = vels[i - 1], biases[i - 1]
        for a in np.nonzero(s["obs_pose"] == i)[0].tolist():
            j = int(s["obs_point"][a])
            if j not in present:
                present.add(j)
                first_seen[j] = i
                points[j] = s["points_init"][j]
            ts[j] = landmark_stamp(j, first_seen[j], i)
            live.add(a)
        win = DenseWindow(oracle, s, G, lo, i, live, prior)
        k = slice(lo, i + 1)
        poses[k], vels[k], biases[k], points[win.lms] = win.optimize(poses[k], vels[k], biases[k], points[win.lms])
        cut = float(i) - lag
        n_exp = sum(1 for q in range(lo, i + 1) if q < cut)
        if n_exp == 0:
            counts.append((0, 0, 0))
            continue
        new_lo = lo + n_exp
        seen = {int(s["obs_point"][a]) for a in live if s["obs_pose"][a] < new_lo}
        gone = {j for j in seen if ts[j] < cut}
        absorbed = {a for a in live if int(s["obs_point"][a]) in gone}
        discarded = {a for a in live if s["obs_pose"][a] < new_lo and a not in absorbed}
        counts.append((n_exp, len(gone), len(discarded)))
        # the sub-problem: up to the last keyframe an absorbed factor touches -- a landmark's sighting, the ImuFactor and
        # bias walk out of the last expired keyframe, the previous prior
        last = max([int(s["obs_pose"][a]) for a in absorbed] + [new_lo] + ([lo + len(prior.x0) - 1] if prior is not None else []))
        sub = DenseWindow(oracle, s, G, lo, last, absorbed, prior, factors_below=new_lo)
        ks = slice(lo, last + 1)
        prior = sub.marginal(poses[ks], vels[ks], biases[ks], points[sub.lms], n_exp)
        live -= absorbed | discarded
        present -= gone
        lo = new_lo
    return poses, vels, biases, lo, counts


def batch_optimum(oracle, s):
    """The full batch of the smoother scene by the same dense optimiser, and the marginal covariance [18 n, 18 n] of its
    camera-side nodes at the optimum."""
    n = len(s["poses_gt"])
    full = DenseWindow(oracle, s, smoother_graph(s), 0, n - 1, range(len(s["obs_pose"])))
    vels = np.tile(s["vels_gt"][0], (n, 1))
    poses, vels, biases, points = full.optimize(s["poses_init"].copy(), vels, np.zeros((n, 6)), s["points_init"].copy(), 60)
    A, _, _ = full.system(poses, vels, biases, points, 0.0)
    return poses, vels, biases, np.linalg.inv(A)
