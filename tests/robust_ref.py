"""Numpy reference of the robust stereo factors (include/vus_robust.h) for the tests: GTSAM's noiseModel::Robust with
Block reweighting applied to the per-observation residuals and Jacobians of the CPU oracle (oracle.stereo_factor), and a
small Levenberg-Marquardt (dense reduced camera system) that follows GTSAM's tryLambda with a fixed lambda factor -- the
loop of ba.py.

Kinds are the VUS_LOSS_* numbers: 0 Gaussian, 1 Huber, 2 Cauchy, 3 Tukey, 4 Geman-McClure, 5 Welsch."""
import math

import numpy as np

KINDS = {"gaussian": 0, "huber": 1, "cauchy": 2, "tukey": 3, "geman_mcclure": 4, "welsch": 5}


def weight_loss(kind, k, d):
    """(w(d), rho(d)) of the table in include/vus_robust.h, elementwise over d >= 0."""
    d = np.asarray(d, dtype=np.float64)
    d2, k2 = d * d, float(k) * float(k)
    if kind == 0:
        return np.ones_like(d), 0.5 * d2
    if kind == 1:
        inl = d <= k
        with np.errstate(divide="ignore"):
            return np.where(inl, 1.0, k / d), np.where(inl, 0.5 * d2, k * d - 0.5 * k2)
    if kind == 2:
        return k2 / (k2 + d2), 0.5 * k2 * np.log1p(d2 / k2)
    if kind == 3:
        t = 1.0 - d2 / k2
        inl = d2 <= k2
        return np.where(inl, t * t, 0.0), np.where(inl, k2 / 6.0 * (1.0 - t * t * t), k2 / 6.0)
    if kind == 4:
        s = k2 + d2
        return k2 * k2 / (s * s), 0.5 * k2 * d2 / s
    if kind == 5:
        return np.exp(-d2 / k2), -0.5 * k2 * np.expm1(-d2 / k2)
    raise ValueError(kind)


class RobustBA:
    """A packed stereo BA problem (numpy L-order arrays of ba_pack.pack_observations) with priors and one loss."""

    def __init__(self, O, pk, K, sigma, kind, k, priors=None):
        self.O = O
        np_ = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        self.nP, self.nL, self.nO = int(pk["n_poses"]), int(pk["n_points"]), int(pk["n_obs"])
        self.op = np_(pk["obs_pose"]).astype(np.int64)
        self.ol = np_(pk["obs_point"]).astype(np.int64)
        self.meas = np.ascontiguousarray(np_(pk["meas"]), dtype=np.float64)
        self.K = np.asarray(K, dtype=np.float64)
        self.w_sig = 1.0 / float(sigma)
        self.kind, self.k = int(kind), float(k)
        if priors is None:
            priors = (np.zeros(0, np.int64), np.zeros((0, 12)), np.zeros((0, 6)))
        self.pr_idx = np.asarray(priors[0], np.int64)
        self.pr_T = np.asarray(priors[1], np.float64).reshape(-1, 12)
        self.pr_w = 1.0 / np.asarray(priors[2], np.float64).reshape(-1, 6)

    # -- per observation --------------------------------------------------------------------------
    def factors(self, poses, points, jac=True):
        """whitened r [n,3], H1 [n,3,6], H2 [n,3,3] from the oracle, L-order"""
        r = np.zeros((self.nO, 3)); H1 = np.zeros((self.nO, 3, 6)); H2 = np.zeros((self.nO, 3, 3))
        for a in range(self.nO):
            r[a], H1[a], H2[a] = self.O.stereo_factor(poses[self.op[a]], points[self.ol[a]], self.meas[a], self.K, self.w_sig)
        return r, H1, H2

    def weights(self, poses, points):
        r, _, _ = self.factors(poses, points)
        return weight_loss(self.kind, self.k, np.sqrt(np.sum(r * r, 1)))[0]

    def _priors(self, poses):
        """whitened prior residuals [n,6] (gtsam PriorFactor: -Local(x, prior)), Jacobian = diag(w)"""
        out = np.zeros((len(self.pr_idx), 6))
        for q, i in enumerate(self.pr_idx):
            out[q] = -self.O.pose_local(poses[i], self.pr_T[q]) * self.pr_w[q]
        return out

    def error(self, poses, points):
        """sum rho(d) over stereo factors + 0.5 |r|^2 over priors: NonlinearFactorGraph.error()"""
        r, _, _ = self.factors(poses, points)
        rho = weight_loss(self.kind, self.k, np.sqrt(np.sum(r * r, 1)))[1]
        return float(np.sum(rho)) + 0.5 * float(np.sum(self._priors(poses) ** 2))

    def linearize(self, poses, points):
        """W [n,18] (H1^T H2, L-order), V [nL,6], gl, Hpp [nP,36], gp, err (0.5 sum w d^2 + priors), w; the reweighted
        per-observation factors are kept for linear_error()."""
        r, H1, H2 = self.factors(poses, points)
        w = weight_loss(self.kind, self.k, np.sqrt(np.sum(r * r, 1)))[0]
        s = np.sqrt(w)
        r, H1, H2 = r * s[:, None], H1 * s[:, None, None], H2 * s[:, None, None]
        self._lin = (r, H1, H2, self._priors(poses))
        W = np.einsum("nki,nkj->nij", H1, H2).reshape(-1, 18)
        V6 = np.einsum("nki,nkj->nij", H2, H2)
        V = np.zeros((self.nL, 6)); gl = np.zeros((self.nL, 3))
        iu = np.triu_indices(3)
        np.add.at(V, self.ol, V6[:, iu[0], iu[1]])
        np.add.at(gl, self.ol, np.einsum("nki,nk->ni", H2, r))
        Hpp = np.zeros((self.nP, 6, 6)); gp = np.zeros((self.nP, 6))
        np.add.at(Hpp, self.op, np.einsum("nki,nkj->nij", H1, H1))
        np.add.at(gp, self.op, np.einsum("nki,nk->ni", H1, r))
        pr = self._lin[3]
        for q, i in enumerate(self.pr_idx):
            Hpp[i] += np.diag(self.pr_w[q] ** 2)
            gp[i] += self.pr_w[q] * pr[q]
        err = 0.5 * float(np.sum(r * r)) + 0.5 * float(np.sum(pr * pr))
        return {"W": W, "V": V, "gl": gl, "Hpp": Hpp.reshape(-1, 36), "gp": gp, "err": err, "w": w}

    def linear_error(self, dp, dl):
        """0.5 sum w |b + J delta|^2 (+ priors) of the last linearize()"""
        r, H1, H2, pr = self._lin
        t = r + np.einsum("nij,nj->ni", H1, dp[self.op]) + np.einsum("nij,nj->ni", H2, dl[self.ol])
        e = 0.5 * float(np.sum(t * t))
        for q, i in enumerate(self.pr_idx):
            e += 0.5 * float(np.sum((pr[q] + self.pr_w[q] * dp[i]) ** 2))
        return e

    def retract(self, poses, points, dp, dl):
        return np.stack([self.O.pose_retract(poses[i], dp[i]) for i in range(self.nP)]), points + dl

    def eval_step(self, poses, points, dp, dl):
        """(new poses, new points, linear error at the step, nonlinear error at the new values)"""
        npo, npt = self.retract(poses, points, dp, dl)
        return npo, npt, self.linear_error(dp, dl), self.error(npo, npt)

    # -- damped solve -------------------------------------------------------------------------------
    def solve(self, lin, lam):
        """(dp [nP,6], dl [nL,3]) of (H + lam I) delta = -g by landmark elimination, as the GPU path does it:
        S = Hpp + lam I - sum W Vinv W^T (dense, Cholesky), dl = -Vinv (gl + sum W^T dp)"""
        nP, nL = self.nP, self.nL
        iu = np.triu_indices(3)
        Vb = np.zeros((nL, 3, 3)); Vb[:, iu[0], iu[1]] = lin["V"]
        Vb = Vb + np.triu(Vb, 1).transpose(0, 2, 1) + lam * np.eye(3)
        Vinv = np.linalg.inv(Vb)
        Wa = lin["W"].reshape(-1, 6, 3)
        Y = np.einsum("nij,njk->nik", Wa, Vinv[self.ol])                 # W Vinv per observation
        S = np.zeros((nP, 6, nP, 6))
        order = np.argsort(self.ol, kind="stable")
        ptr = np.searchsorted(self.ol[order], np.arange(nL + 1))
        for j in range(nL):
            a = order[ptr[j]:ptr[j + 1]]
            for x in a:
                for y in a:
                    S[self.op[x], :, self.op[y], :] -= Y[x] @ Wa[y].T
        S = S.reshape(6 * nP, 6 * nP)
        for i in range(nP):
            S[6 * i:6 * i + 6, 6 * i:6 * i + 6] += lin["Hpp"][i].reshape(6, 6) + lam * np.eye(6)
        gs = lin["gp"].copy()
        np.add.at(gs, self.op, -np.einsum("nij,nj->ni", Y, lin["gl"][self.ol]))
        if "pose_H" in lin:         # further factors on poses alone (between factors), undamped: [6 nP]^2 and [6 nP]
            S = S + lin["pose_H"]
            gs = gs + lin["pose_g"].reshape(nP, 6)
        Lc = np.linalg.cholesky(S)
        dp = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, gs.reshape(-1))).reshape(nP, 6)
        t = lin["gl"].copy()
        np.add.at(t, self.ol, np.einsum("nij,ni->nj", Wa, dp[self.op]))
        dl = -np.einsum("nij,nj->ni", Vinv, t)
        return dp, dl

    def lm(self, poses, points, lambdaInitial=1e-5, lambdaFactor=10.0, lambdaUpperBound=1e5, lambdaLowerBound=0.0,
           minModelFidelity=1e-3, maxIterations=100, relativeErrorTol=1e-5, absoluteErrorTol=1e-5, errorTol=0.0):
        """GTSAM's LevenbergMarquardtOptimizer (iterate / tryLambda / checkConvergence, fixed lambda factor), as ba.py's
        StereoBASolver.optimize runs it.  Returns (poses, points, report dict of oracle.ba_lm_optimize's shape)."""
        poses, points = np.array(poses, dtype=np.float64), np.array(points, dtype=np.float64)
        rep = {"iterations": 0, "outer": 0, "tries": 0, "status": 1, "err_hist": [], "lambda_hist": []}
        lam = lambdaInitial
        current = self.error(poses, points)
        rep["initial_error"] = current
        if current <= errorTol or maxIterations <= 0:       # before the first iteration: converged / max iterations
            rep.update(status=0 if current <= errorTol else 1, final_error=current, final_lambda=lam)
            return poses, points, rep
        while rep["iterations"] < maxIterations:
            lin = self.linearize(poses, points)
            lin0 = lin["err"]
            new_error, stop_search, accepted = current, False, False
            while True:
                dp, dl = self.solve(lin, lam)
                npo, npt, lin1, new1 = self.eval_step(poses, points, dp, dl)
                rep["tries"] += 1
                success = False
                if math.isfinite(lin1) and math.isfinite(new1):
                    lin_change = lin0 - lin1
                    if lin_change >= 0.0:
                        cost_change = current - new1
                        if lin_change > 2.220446049250313e-16 * lin0:
                            success = cost_change / lin_change > minModelFidelity
                        if abs(cost_change) < relativeErrorTol * current:
                            stop_search = True
                        if success:
                            poses, points, new_error = npo, npt, new1
                if success:
                    lam = max(lambdaLowerBound, lam / lambdaFactor)
                    accepted = True
                    break
                if stop_search:
                    break
                lam *= lambdaFactor
                if lam >= lambdaUpperBound:
                    rep["status"] = 2
                    break
            rep["err_hist"].append(new_error)
            rep["lambda_hist"].append(lam)
            rep["outer"] += 1
            rep["iterations"] += int(accepted)
            if new_error <= errorTol:
                converged = True
            else:
                abs_dec = current - new_error
                converged = (abs_dec / current <= relativeErrorTol) or (abs_dec <= absoluteErrorTol)
            current = new_error
            if rep["status"] == 2:
                break
            if converged:
                rep["status"] = 0
                break
            if not math.isfinite(current):
                break
        rep["final_error"], rep["final_lambda"] = current, lam
        return poses, points, rep
