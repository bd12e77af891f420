"""numpy statement of the marginal covariances (include/vus_marginals.h): the blocked selected inversion of a block band,
the landmark formula and the shared-bias border correction.  Test infrastructure only."""
import numpy as np

PB = 8      # nodes per panel


def band_to_dense(Sb):
    """Symmetric dense matrix of a block band [n, band + 1, 36] (lower blocks stored)."""
    n, B1 = Sb.shape[0], Sb.shape[1]
    A = np.zeros((6 * n, 6 * n))
    for i in range(n):
        for s in range(min(B1, i + 1)):
            k = i - s
            blk = Sb[i, s].reshape(6, 6)
            A[6 * i:6 * i + 6, 6 * k:6 * k + 6] = blk
            if s:
                A[6 * k:6 * k + 6, 6 * i:6 * i + 6] = blk.T
    return A


def dense_to_band(A, band):
    n = A.shape[0] // 6
    Sb = np.zeros((n, band + 1, 36))
    for i in range(n):
        for s in range(min(band + 1, i + 1)):
            k = i - s
            Sb[i, s] = A[6 * i:6 * i + 6, 6 * k:6 * k + 6].reshape(-1)
    return Sb


def random_spd_band(rng, n, band):
    """A random SPD block band of n nodes and half-bandwidth `band` nodes: (dense, band storage)."""
    A = np.zeros((6 * n, 6 * n))
    for i in range(n):
        for k in range(max(0, i - band), i + 1):
            A[6 * i:6 * i + 6, 6 * k:6 * k + 6] = rng.normal(size=(6, 6))
    A = np.tril(A) + np.tril(A, -1).T
    A += np.eye(6 * n) * (np.abs(A).sum(1).max() + 1.0)
    return A, dense_to_band(A, band)


def selinv_band(A, band):
    """The band of A^-1 by the panel recursion of vus_ba_band_selinv, from the Cholesky factor only:
    bottom-up over 8-node panels P with the rows R = the `band` nodes below them,
        X = L_RP L_PP^-1,  Sigma_RP = -Sigma_RR X,  Sigma_PP = L_PP^-T L_PP^-1 - X^T Sigma_RP.
    Sigma_RR is read only where the band stores it (|i - j| < band); Sigma_RP is kept whole for the step and only its
    part inside the band is stored.  Returns the band storage [n, band + 1, 36] (slots left of column 0 zero)."""
    n = A.shape[0] // 6
    L = np.linalg.cholesky(A)
    Sg = np.zeros((n, band + 1, 36))

    def get(i, j):          # Sigma(i, j) from the band (i, j within band - 1 of each other)
        if i >= j:
            assert i - j <= band
            return Sg[i, i - j].reshape(6, 6)
        return get(j, i).T

    for k0 in range(PB * ((n - 1) // PB), -1, -PB):
        nb = min(PB, n - k0)
        P = slice(6 * k0, 6 * (k0 + nb))
        r0, r1 = k0 + nb, min(n, k0 + PB + band)
        Li = np.linalg.inv(L[P, P])
        if r1 > r0:
            R = slice(6 * r0, 6 * r1)
            X = L[R, P] @ Li
            SRR = np.zeros((6 * (r1 - r0),) * 2)
            for a in range(r0, r1):
                for b in range(r0, r1):
                    SRR[6 * (a - r0):6 * (a - r0) + 6, 6 * (b - r0):6 * (b - r0) + 6] = get(a, b)
            SRP = -SRR @ X
            SPP = Li.T @ Li - X.T @ SRP
            for a in range(r0, r1):
                for kk in range(nb):
                    if a - (k0 + kk) <= band:
                        Sg[a, a - k0 - kk] = SRP[6 * (a - r0):6 * (a - r0) + 6, 6 * kk:6 * kk + 6].reshape(-1)
        else:
            SPP = Li.T @ Li
        SPP = 0.5 * (SPP + SPP.T)
        for a in range(nb):
            for b in range(a + 1):
                if a - b <= band:
                    Sg[k0 + a, a - b] = SPP[6 * a:6 * a + 6, 6 * b:6 * b + 6].reshape(-1)
    return Sg


def sym3(v):
    """3 x 3 from the upper triangle (xx, xy, xz, yy, yz, zz)."""
    a, b, c, d, e, f = v
    return np.array([[a, b, c], [b, d, e], [c, e, f]])


def point_covariance(Sigma_of, W, V, obs_pose, obs_point, n_points, ps=1):
    """cov_j = V_j^-1 + sum_{a, b observing j} Y_a^T Sigma(node_a, node_b) Y_b with Y = W V^-1 (lambda = 0);
    Sigma_of(i, k) returns the 6 x 6 camera-side covariance block of nodes i, k."""
    cov = np.zeros((n_points, 3, 3))
    for j in range(n_points):
        rows = np.nonzero(obs_point == j)[0]
        Vi = np.linalg.inv(sym3(V[j]))
        Y = [W[o].reshape(6, 3) @ Vi for o in rows]
        c = Vi.copy()
        for a, oa in enumerate(rows):
            for b, ob in enumerate(rows):
                c += Y[a].T @ Sigma_of(ps * obs_pose[oa], ps * obs_pose[ob]) @ Y[b]
        cov[j] = c
    return cov


def border_correction(Ainv, Scb, Sbb):
    """Camera-side system A with the shared-bias border (Scb [6n, 6], Sbb [6, 6]):
    U = A^-1 Scb, Sc = Sbb - Scb^T U; returns (Sigma_cc = A^-1 + U Sc^-1 U^T, Sigma_cb = -U Sc^-1, Sigma_bb = Sc^-1)."""
    U = Ainv @ Scb
    Sci = np.linalg.inv(Sbb - Scb.T @ U)
    return Ainv + U @ Sci @ U.T, -U @ Sci, Sci
