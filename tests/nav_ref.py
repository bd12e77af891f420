"""Dense f64 reference of the inertial full-graph camera system (NavBASolver): the reduced system over the camera-side
nodes (node 2i = pose i, node 2i + 1 = velocity i padded to 6) and the shared-bias border, 6 n_nodes + 6 unknowns,
assembled block by block from the oracle twins only -- vus_ba_linearize_cpu / vus_ba_schur_cpu for the stereo Schur
complement, vus_nav_linearize_cpu for the inertial blocks.  Independent of the kernels' band layout code.
Test infrastructure only (a plain module, not a conftest)."""
import numpy as np


def pose_band(obs_pose, obs_point):
    """Widest keyframe span of a landmark (obs rows sorted by landmark, as synth emits them)."""
    obs_pose, obs_point = np.asarray(obs_pose), np.asarray(obs_point)
    if len(obs_pose) == 0:
        return 0
    hi, lo = np.zeros(obs_point.max() + 1, np.int64), np.full(obs_point.max() + 1, np.iinfo(np.int64).max)
    np.maximum.at(hi, obs_point, obs_pose)
    np.minimum.at(lo, obs_point, obs_pose)
    seen = lo <= hi
    return int((hi[seen] - lo[seen]).max())


def nav_linearize(oracle, N, poses, vels, bias):
    """vus_nav_linearize_cpu: Snav [n_nodes, 4, 36], Scb [n_nodes, 36], Sbb [36], gnav [n_nodes, 6], gb [6], err."""
    nP = len(poses)
    nN = 2 * nP
    out = {"Snav": np.zeros((nN, 4, 36)), "Scb": np.zeros((nN, 36)), "Sbb": np.zeros(36), "gnav": np.zeros((nN, 6)),
           "gb": np.zeros(6)}
    e = np.zeros(1)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    rc = oracle.lib().vus_nav_linearize_cpu(N.ref(), nP, oracle._p(f(poses)), oracle._p(f(vels)), oracle._p(f(bias)),
                                            *[oracle._p(out[k]) for k in ("Snav", "Scb", "Sbb", "gnav", "gb")],
                                            oracle._p(e), None)
    assert rc == 0
    out["err"] = float(e[0])
    return out


def dense_system(oracle, s, P, N, poses, vels, bias, points, lam):
    """The bordered camera system at (poses, vels, bias, points) and damping lam, as the solver builds it:
      A     [6 n_nodes + 6]^2  stereo Schur complement (V + lam I eliminated, lam I on the pose blocks) scattered to the
                               even nodes, plus the inertial blocks, lam on the 3 real and 1 on the 3 padding coordinates
                               of every velocity node, and the border [[A_cc, Scb], [Scb^T, Sbb + lam I]]
      g     [6 n_nodes + 6]    the reduced gradient (the step solves A x = -g)
      err                      the error at the linearisation point (stereo + priors + inertial)
    and the pieces: gcam (the gradient before the landmarks are eliminated), lin (oracle.ba_linearize), sch
    (oracle.ba_schur), nav (nav_linearize) and the pose band used."""
    nP = len(poses)
    nN, nc = 2 * nP, 12 * nP
    lin = oracle.ba_linearize(P, poses, points)
    band = pose_band(s["obs_pose"], s["obs_point"])
    sch = oracle.ba_schur(P, band, lam, lin)
    nav = nav_linearize(oracle, N, poses, vels, bias)
    A = np.zeros((nc + 6, nc + 6))
    g = np.zeros(nc + 6)
    gcam = np.zeros(nc + 6)
    for i in range(nP):             # stereo: pose i is node 2i
        for sl in range(min(i, band) + 1):
            blk = sch["Sband"][i, sl].reshape(6, 6)
            k = i - sl
            A[12 * i:12 * i + 6, 12 * k:12 * k + 6] += blk
            if sl:
                A[12 * k:12 * k + 6, 12 * i:12 * i + 6] += blk.T
        g[12 * i:12 * i + 6] = sch["gs"][i]
        gcam[12 * i:12 * i + 6] = lin["gp"][i]
    Snav = nav["Snav"]
    for node in range(nN):          # inertial: nodes 3 apart at most
        for sl in range(min(node, 3) + 1):
            blk = Snav[node, sl].reshape(6, 6)
            k = node - sl
            A[6 * node:6 * node + 6, 6 * k:6 * k + 6] += blk
            if sl:
                A[6 * k:6 * k + 6, 6 * node:6 * node + 6] += blk.T
        if node & 1:
            for dim in range(6):
                A[6 * node + dim, 6 * node + dim] += lam if dim < 3 else 1.0
    g[:nc] += nav["gnav"].reshape(-1)
    gcam[:nc] += nav["gnav"].reshape(-1)
    C = nav["Scb"].reshape(nN, 6, 6).reshape(nc, 6)
    A[:nc, nc:] = C
    A[nc:, :nc] = C.T
    A[nc:, nc:] = nav["Sbb"].reshape(6, 6) + lam * np.eye(6)
    g[nc:] = gcam[nc:] = nav["gb"]
    return {"A": A, "g": g, "err": lin["err"] + nav["err"], "gcam": gcam, "lin": lin, "sch": sch, "nav": nav,
            "band": band}


def split_step(x, n_poses):
    """Camera-side step (6 n_nodes + 6) -> (pose steps [n,6], velocity steps [n,3], velocity padding [n,3], bias step)."""
    nodes = x[:12 * n_poses].reshape(n_poses, 2, 6)
    return nodes[:, 0], nodes[:, 1, :3], nodes[:, 1, 3:], x[12 * n_poses:]


def retract(oracle, poses, vels, bias, x):
    """The solver's retraction of a camera-side step: poses by vus_pose_retract_cpu, velocities and bias additively."""
    dp, dv, _, db = split_step(x, len(poses))
    return (np.stack([oracle.pose_retract(poses[i], dp[i]) for i in range(len(poses))]), vels + dv, bias + db)


def solve(A, rhs):
    """Cholesky solve of the SPD system.  Returns (x, kappa, d): d = sqrt(diag A), kappa = the 1-norm condition number
    estimate (LAPACK dpocon) of the Jacobi-scaled matrix D^-1 A D^-1.  A Cholesky solve is invariant to that scaling, so
    its error is bounded in the scaled unknowns: |d (x_hat - x)| / |d x| <~ c kappa eps (van der Sluis)."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.linalg.lapack import dpocon
    d = np.sqrt(np.diag(A))
    As = A / d[:, None] / d[None, :]
    c, low = cho_factor(As, lower=True)
    rcond, info = dpocon(c, np.abs(As).sum(0).max(), uplo="L")
    assert info == 0
    return cho_solve((c, low), rhs / d[:, None] if rhs.ndim == 2 else rhs / d) / (d[:, None] if rhs.ndim == 2 else d), 1.0 / rcond, d


def scaled_err(x, ref, d):
    """max |d (x - ref)| / max |d ref|: the error measure of solve()'s bound."""
    return float(np.abs(d * (x - ref)).max() / np.abs(d * ref).max())
