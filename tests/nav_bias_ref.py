"""Dense f64 reference of the inertial camera system with ONE IMU BIAS PER KEYFRAME (NavBiasBASolver): the reduced system
over the camera-side nodes (node 3i = pose i, 3i + 1 = velocity i padded to 6, 3i + 2 = bias i), 6 * 3n unknowns and no
border, assembled block by block from the oracle twins only -- vus_ba_linearize_cpu / vus_ba_schur_cpu for the stereo
Schur complement, vus_imu_factor_cpu per ImuFactor at that factor's own bias, vus_dvl_factor_cpu -- and numpy for the
bias between-factors and priors.  Also a dense LM that takes the oracle LM's trials and lambda rules.
Test infrastructure only (a plain module, not a conftest)."""
import math

import numpy as np

from nav_ref import pose_band, solve, scaled_err  # noqa: F401  (re-exported for the tests)


class BiasGraph:
    """Host-side description of the inertial factors: imu = (i [n], pim [n,148], W [n,81]) with j = i + 1, dvl = (pose,
    meas [n,3], sigma [n]), vprior = (idx, v [n,3], sigmas [n,3]), bbetween = (i, meas [n,6], sigmas [n,6]) with
    j = i + 1, bprior = (idx, mean [n,6], sigmas [n,6])."""

    def __init__(self, gravity, imu=None, dvl=None, vprior=None, bbetween=None, bprior=None):
        e = lambda k, shape: np.zeros(shape)
        self.g = np.asarray(gravity, float)
        self.imu_i = np.asarray(imu[0], np.int64) if imu else np.zeros(0, np.int64)
        self.imu_pim = np.asarray(imu[1], float).reshape(-1, 148) if imu else e(0, (0, 148))
        self.imu_W = np.asarray(imu[2], float).reshape(-1, 9, 9) if imu else e(0, (0, 9, 9))
        self.dvl_pose = np.asarray(dvl[0], np.int64) if dvl else np.zeros(0, np.int64)
        self.dvl_meas = np.asarray(dvl[1], float).reshape(-1, 3) if dvl else e(0, (0, 3))
        self.dvl_w = 1.0 / np.asarray(dvl[2], float).reshape(-1) if dvl else e(0, (0,))
        self.vp_idx = np.asarray(vprior[0], np.int64) if vprior else np.zeros(0, np.int64)
        self.vp_v = np.asarray(vprior[1], float).reshape(-1, 3) if vprior else e(0, (0, 3))
        self.vp_w = 1.0 / np.asarray(vprior[2], float).reshape(-1, 3) if vprior else e(0, (0, 3))
        self.bb_i = np.asarray(bbetween[0], np.int64) if bbetween else np.zeros(0, np.int64)
        self.bb_meas = np.asarray(bbetween[1], float).reshape(-1, 6) if bbetween else e(0, (0, 6))
        self.bb_w = 1.0 / np.asarray(bbetween[2], float).reshape(-1, 6) if bbetween else e(0, (0, 6))
        self.bp_idx = np.asarray(bprior[0], np.int64) if bprior else np.zeros(0, np.int64)
        self.bp_mean = np.asarray(bprior[1], float).reshape(-1, 6) if bprior else e(0, (0, 6))
        self.bp_w = 1.0 / np.asarray(bprior[2], float).reshape(-1, 6) if bprior else e(0, (0, 6))

    def device(self, device="cuda:0"):
        """The same factors as the solver's NavBiasFactors."""
        from visual_underwater_slam_amd.ba import NavBiasFactors
        ii, bi = self.imu_i, self.bb_i
        return NavBiasFactors(self.g, imu=(ii, ii + 1, self.imu_pim, self.imu_W.reshape(-1, 81)) if len(ii) else None,
                              dvl=(self.dvl_pose, self.dvl_meas, 1.0 / self.dvl_w) if len(self.dvl_pose) else None,
                              vprior=(self.vp_idx, self.vp_v, 1.0 / self.vp_w) if len(self.vp_idx) else None,
                              bbetween=(bi, bi + 1, self.bb_meas, 1.0 / self.bb_w) if len(bi) else None,
                              bprior=(self.bp_idx, self.bp_mean, 1.0 / self.bp_w) if len(self.bp_idx) else None,
                              device=device)


def _factors(oracle, G, poses, vels, biases):
    """Every inertial factor's whitened residual and Jacobian: list of (rw [m], [(node, Jw [m, 6 or 3], dims)])."""
    out = []
    for f, i in enumerate(G.imu_i):
        j = i + 1
        r, J = oracle.imu_factor(poses[i], vels[i], poses[j], vels[j], biases[i], G.imu_pim[f], G.g)
        W = G.imu_W[f]
        rw, Jw = W @ r, W @ J
        out.append((rw, [(3 * i, Jw[:, 0:6]), (3 * i + 1, Jw[:, 6:9]), (3 * j, Jw[:, 9:15]), (3 * j + 1, Jw[:, 15:18]),
                         (3 * i + 2, Jw[:, 18:24])]))
    for f, i in enumerate(G.dvl_pose):
        e, JX, Jv = oracle.dvl_factor(poses[i], vels[i], G.dvl_meas[f])
        w = G.dvl_w[f]
        out.append((w * e, [(3 * i, w * JX), (3 * i + 1, w * Jv)]))
    for f, i in enumerate(G.vp_idx):
        w = G.vp_w[f]
        out.append((w * (vels[i] - G.vp_v[f]), [(3 * i + 1, np.diag(w))]))
    for f, i in enumerate(G.bb_i):
        w = G.bb_w[f]
        out.append((w * (biases[i + 1] - biases[i] - G.bb_meas[f]), [(3 * i + 2, -np.diag(w)), (3 * i + 5, np.diag(w))]))
    for f, i in enumerate(G.bp_idx):
        w = G.bp_w[f]
        out.append((w * (biases[i] - G.bp_mean[f]), [(3 * i + 2, np.diag(w))]))
    return out


def inertial_error(oracle, G, poses, vels, biases):
    return sum(0.5 * float(rw @ rw) for rw, _ in _factors(oracle, G, poses, vels, biases))


def total_error(oracle, P, G, poses, vels, biases, points):
    return oracle.ba_error(P, poses, points) + inertial_error(oracle, G, poses, vels, biases)


def inertial_system(oracle, G, poses, vels, biases):
    """The inertial factors' undamped normal equations over the nodes: H [18n, 18n], g [18n], err, and the factors."""
    n = len(poses)
    H, g, err = np.zeros((18 * n, 18 * n)), np.zeros(18 * n), 0.0
    fac = _factors(oracle, G, poses, vels, biases)
    for rw, cols in fac:
        err += 0.5 * float(rw @ rw)
        for na, Ja in cols:
            ca = 6 * na
            g[ca:ca + Ja.shape[1]] += Ja.T @ rw
            for nb, Jb in cols:
                cb = 6 * nb
                H[ca:ca + Ja.shape[1], cb:cb + Jb.shape[1]] += Ja.T @ Jb
    return H, g, err, fac


def dense_system(oracle, s, P, G, poses, vels, biases, points, lam, band=None):
    """The camera system at (poses, vels, biases, points) and damping lam, as the solver builds it:
      A [18n, 18n]  stereo Schur complement (V + lam I eliminated, lam I on the pose blocks) scattered to nodes 3i, plus
                    the inertial blocks, lam on the 3 real and 1 on the 3 padding coordinates of every velocity node and
                    lam on every bias node
      g [18n]       the reduced gradient (the step solves A x = -g)
    plus err (stereo + priors + inertial at the linearisation point), the inertial part (Hnav, gnav, nav_err) and the
    oracle's stereo pieces lin / sch."""
    n = len(poses)
    lin = oracle.ba_linearize(P, poses, points)
    band = pose_band(s["obs_pose"], s["obs_point"]) if band is None else band
    sch = oracle.ba_schur(P, band, lam, lin)
    Hn, gn, en, fac = inertial_system(oracle, G, poses, vels, biases)
    A, g = Hn.copy(), gn.copy()
    for i in range(n):
        for sl in range(min(i, band) + 1):
            blk = sch["Sband"][i, sl].reshape(6, 6)
            k = i - sl
            A[18 * i:18 * i + 6, 18 * k:18 * k + 6] += blk
            if sl:
                A[18 * k:18 * k + 6, 18 * i:18 * i + 6] += blk.T
        g[18 * i:18 * i + 6] += sch["gs"][i]
        for dim in range(6):
            A[18 * i + 6 + dim, 18 * i + 6 + dim] += lam if dim < 3 else 1.0
            A[18 * i + 12 + dim, 18 * i + 12 + dim] += lam
    gcam = gn.copy()
    for i in range(n):
        gcam[18 * i:18 * i + 6] += lin["gp"][i]
    return {"A": A, "g": g, "gcam": gcam, "err": lin["err"] + en, "Hnav": Hn, "gnav": gn, "nav_err": en, "lin": lin,
            "sch": sch, "band": band, "factors": fac}


def split_step(x, n):
    """Node step [18n] -> (pose steps [n,6], velocity steps [n,3], velocity padding [n,3], bias steps [n,6])."""
    nodes = x.reshape(n, 3, 6)
    return nodes[:, 0], nodes[:, 1, :3], nodes[:, 1, 3:], nodes[:, 2]


def retract(oracle, poses, vels, biases, x):
    dp, dv, _, db = split_step(x, len(poses))
    return np.stack([oracle.pose_retract(poses[i], dp[i]) for i in range(len(poses))]), vels + dv, biases + db


def band_blocks(A, n_nodes, band, diagonals=None):
    """The dense matrix's blocks (node, node - s), s = 0..band, as [n_nodes, band + 1, 36] (zero left of column 0)."""
    nd = band + 1 if diagonals is None else diagonals
    out = np.zeros((n_nodes, nd, 36))
    for q in range(n_nodes):
        for sl in range(min(q, nd - 1) + 1):
            out[q, sl] = A[6 * q:6 * q + 6, 6 * (q - sl):6 * (q - sl) + 6].reshape(-1)
    return out


def lm_trial(oracle, s, P, G, poses, vels, biases, points, lam, cholesky=False):
    """One damped trial of the dense LM at (poses, vels, biases, points): solves the dense camera system (LU; `cholesky`:
    solve()'s Cholesky of the Jacobi-scaled matrix, a second rounding of the same step), back-substitutes the landmarks
    (vus_ba_backsub_cpu), takes the stereo linearised and new errors from vus_ba_eval_step_cpu and the inertial ones from
    the factors.  Returns (lin0, lin1, new1, the trial state)."""
    n = len(poses)
    ref = dense_system(oracle, s, P, G, poses, vels, biases, points, lam)
    x = solve(ref["A"], -ref["g"])[0] if cholesky else np.linalg.solve(ref["A"], -ref["g"])
    dp, dv, _, db = split_step(x, n)
    dl = oracle.ba_backsub(P, ref["lin"], ref["sch"]["Vinv"], dp)
    npo, npt, lin_s, new_s = oracle.ba_eval_step(P, poses, points, dp, dl)
    lin_n = 0.0
    for rw, cols in ref["factors"]:
        r = rw.copy()
        for node, J in cols:
            r += J @ x[6 * node:6 * node + J.shape[1]]
        lin_n += 0.5 * float(r @ r)
    nv, nb = vels + dv, biases + db
    new_n = inertial_error(oracle, G, npo, nv, nb)
    return ref["err"], lin_s + lin_n, new_s + new_n, (npo, nv, nb, npt)


def lm_optimize(oracle, s, P, G, poses, vels, biases, points, max_iterations=100, lambda_initial=1e-5, lambda_factor=10.0,
                lambda_upper=1e5, lambda_lower=0.0, min_model_fidelity=1e-3, rel_tol=1e-5, abs_tol=1e-5, error_tol=0.0):
    """Dense LM with the oracle LM's iterate / tryLambda / convergence rules (GTSAM's defaults) over lm_trial().  Returns
    the state and a report with the oracle's keys plus `trials` = [(lambda, accepted)]."""
    poses, vels, biases, points = (np.array(a, float, copy=True) for a in (poses, vels, biases, points))
    rep = {"iterations": 0, "outer": 0, "tries": 0, "status": 1, "err_hist": [], "lambda_hist": [], "trials": []}
    lam = lambda_initial
    current = total_error(oracle, P, G, poses, vels, biases, points)
    rep["initial_error"] = current
    at_tol = current <= error_tol           # before the first iteration: converged, the state untouched
    if at_tol:
        rep["status"] = 0
    while not at_tol and rep["iterations"] < max_iterations:
        new_error, stop, accepted = current, False, False
        while True:
            lin0, lin1, new1, trial = lm_trial(oracle, s, P, G, poses, vels, biases, points, lam)
            rep["tries"] += 1
            success = False
            if math.isfinite(lin1) and math.isfinite(new1):
                lin_change = lin0 - lin1
                if lin_change >= 0.0:
                    cost_change = current - new1
                    if lin_change > 2.220446049250313e-16 * lin0:
                        success = cost_change / lin_change > min_model_fidelity
                    if abs(cost_change) < rel_tol * current:
                        stop = True
                    if success:
                        (poses, vels, biases, points), new_error = trial, new1
            rep["trials"].append((lam, success))
            if success:
                lam = max(lambda_lower, lam / lambda_factor)
                accepted = True
                break
            if stop:
                break
            lam *= lambda_factor
            if lam >= lambda_upper:
                rep["status"] = 2
                break
        rep["err_hist"].append(new_error)
        rep["lambda_hist"].append(lam)
        rep["outer"] += 1
        rep["iterations"] += int(accepted)
        if new_error <= error_tol:
            converged = True
        else:
            dec = current - new_error
            converged = dec / current <= rel_tol or dec <= abs_tol
        current = new_error
        if rep["status"] == 2 or converged or not math.isfinite(current):
            if converged and rep["status"] != 2:
                rep["status"] = 0
            break
    rep["final_error"], rep["final_lambda"] = current, lam
    return poses, vels, biases, points, rep


ACC_COV = np.eye(3) * 8.999999999999999e-08      # the covariances of test_nav_oracle (batch.py:183-185)
GYRO_COV = np.eye(3) * 1.2184696791468346e-07
INT_COV = np.eye(3) * 1e-07


def preintegrate(s):
    """(pim [n-1, 148], W [n-1, 81]) of every keyframe interval of a nav_sequence, at a zero bias estimate."""
    from visual_underwater_slam_amd.gtsam.imu import Preintegrator
    pims, Ws = [], []
    for samples in s["imu"]:
        pre = Preintegrator(np.zeros(6), ACC_COV, GYRO_COV, INT_COV)
        for smp in samples:
            pre.integrate(smp[:3], smp[3:6], smp[6])
        pims.append(pre.packed()); Ws.append(pre.whitening().reshape(-1))
    return np.array(pims).reshape(-1, 148), np.array(Ws).reshape(-1, 81)


def make_graph(oracle, s, rw_sigma=(1e-2, 1e-3), bias_prior_sigma=(0.1, 0.01), dvl_poses=None, vprior_truth=False,
               with_between=True, with_prior=True):
    """Oracle stereo problem + BiasGraph of a nav_sequence: pose prior on X(0), ImuFactor(X(i), V(i), X(i+1), V(i+1), B(i))
    for every interval, BetweenFactorConstantBias(B(i), B(i+1), 0, rw_sigma * sqrt(dt)), a zero-mean prior on B(0),
    DVL on `dvl_poses` (default 1 .. n-1; () for none), the prior on V(0) (zero, or the truth)."""
    import torch
    from visual_underwater_slam_amd import ba_pack
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                   torch.from_numpy(s["meas"]), n, nL)
    P = oracle.BAProblem(pk, s["K"], s["sigma"], (np.array([0], np.int32), s["poses_gt"][:1], s["prior_sigmas"][None]))
    pims, Ws = preintegrate(s)
    dt = float(s["imu"][0, :, 6].sum()) if n > 1 else 0.2
    sig = np.repeat(np.asarray(rw_sigma, float), 3) * math.sqrt(dt)
    dp = np.arange(1, n) if dvl_poses is None else np.asarray(dvl_poses, np.int64)
    G = BiasGraph(s["gravity"], imu=(np.arange(n - 1), pims, Ws) if n > 1 else None,
                  dvl=(dp, s["dvl"][dp], np.full(len(dp), 0.1)) if len(dp) else None,
                  vprior=(np.array([0]), s["vels_gt"][:1] * (1.0 if vprior_truth else 0.0), np.full((1, 3), 0.1)),
                  bbetween=(np.arange(n - 1), np.zeros((n - 1, 6)), np.tile(sig, (n - 1, 1))) if n > 1 and with_between else None,
                  bprior=(np.array([0]), np.zeros((1, 6)), np.repeat(np.asarray(bias_prior_sigma, float), 3)[None])
                  if with_prior else None)
    return P, G


def solver(s, G, loss=None, device="cuda:0"):
    """The GPU problem (pose_stride 3) and NavBiasBASolver of the same graph."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBiasBASolver
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    prob = StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                           prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=3, device=device,
                           loss=loss)
    return prob, NavBiasBASolver(prob, G.device(device))
