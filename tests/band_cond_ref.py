"""CPU reference for the band solver's numerics (tests/test_band_cond_ref.py, tests/test_band_cond_gpu.py): seeded families of
ill-conditioned, badly scaled and indefinite block bands, a refined reference solve, the error measures and the assertions
both test files share.  Test infrastructure only: numpy, scipy and mpmath.

Families (6 x 6 blocks, the [n, band + 1, 36] layout of marginals_ref):
  chain(n, band, tau, where)   pose-graph Laplacian with the exact 6-dimensional gauge null space of a chain, held by the
                               prior tau I on pose 0 ("first") or on every pose ("all": LM damping)
  units(A, decades)            D A D, D = diag(1, 1, 1, 10^-d, 10^-d, 10^-d) per pose: rotation against translation scale
  pow4(A, k)                   A 4^k (with b 2^k): every square root, product and reciprocal scales exactly
  indefinite(A, c)             pivot c becomes -L_cc^2, pivots 0 .. c-1 stay
All error measures are taken on the symmetrically equilibrated system (D = diag A):
  A^ = D^-1/2 A D^-1/2,  x^ = D^1/2 x,  b^ = D^-1/2 b
with residuals in np.longdouble."""
import functools

import numpy as np
import scipy.linalg

from marginals_ref import band_to_dense, dense_to_band  # noqa: F401  (re-exported for the tests)

LD = np.longdouble
EPS = 2.0 ** -52
TAUS = (1e-2, 1e-5, 1e-8)
WHERES = ("first", "all")
SHAPES = ((9, 2), (23, 7), (57, 1), (40, 30), (64, 20), (131, 37))
N_RHS = 7


# ---------------------------------------------------------------------------------------------- families
def chain(n, band, tau, where, isolated=None, seed=0):
    """Dense f64 matrix of the chain family.  Every pair i > k >= i - band adds J^T J with J = [J_i, -J_i],
    J_i = I + 0.3 N(0, 1): the pair i - k = 1 always, the others with probability 1/2.  Accumulated in np.longdouble and
    rounded once.  `isolated`: a pose that takes part in no factor and gets no prior (its block row and column are zero)."""
    assert where in WHERES
    rng = np.random.default_rng([seed, n, band, int(round(-np.log10(tau))), WHERES.index(where)])
    A = np.zeros((6 * n, 6 * n), dtype=LD)
    for i in range(1, n):
        for k in range(max(0, i - band), i):
            Ji = (np.eye(6) + 0.3 * rng.normal(size=(6, 6))).astype(LD)
            keep = (i - k == 1) or rng.random() < 0.5
            if not keep or isolated in (i, k):
                continue
            M = Ji.T @ Ji
            M = 0.5 * (M + M.T)
            si, sk = slice(6 * i, 6 * i + 6), slice(6 * k, 6 * k + 6)
            A[si, si] += M
            A[sk, sk] += M
            A[si, sk] -= M
            A[sk, si] -= M
    for p in (range(n) if where == "all" else (0,)):
        if p != isolated:
            A[6 * p:6 * p + 6, 6 * p:6 * p + 6] += LD(tau) * np.eye(6, dtype=LD)
    return np.asarray(A, dtype=np.float64)


def units(A, decades):
    d = np.tile(np.concatenate([np.ones(3, LD), np.full(3, LD(10) ** -decades)]), A.shape[0] // 6)
    return np.asarray(d[:, None] * A.astype(LD) * d[None, :], dtype=np.float64)


def pow4(A, b, k):
    """(A 4^k, b 2^k): exact scalings by powers of two."""
    return np.ldexp(A, 2 * k), np.ldexp(b, k)


def indefinite(A, c, L=None):
    """A with 2 L_cc^2 subtracted from A[c, c] (L the reference factor of the SPD A): pivot c becomes -L_cc^2."""
    L = np.linalg.cholesky(A) if L is None else L
    out = A.copy()
    out[c, c] -= 2.0 * L[c, c] ** 2
    return out


def with_nan(A, r, c):
    out = A.copy()
    out[r, c] = out[c, r] = np.nan
    return out


def nan_positions(n, band):
    """Two sub-diagonal scalar entries (r, c) inside the band: one inside a diagonal block, one `band` poses off it."""
    p = n // 2
    q = min(n - 1, p + band)
    return [(6 * p + 4, 6 * p + 1), (6 * q + 2, 6 * p + 3)]


# ---------------------------------------------------------------------------------------------- reference solves
def lapack_solve(A, B):
    """f64 LAPACK Cholesky solve of A X = B (B [N] or [N, k])."""
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), B)


def lapack_status(A):
    """LAPACK's info of dpotrf: 0, or the order of the leading minor that is not positive definite -- the project's status
    convention (scalar column c -> c + 1)."""
    _, info = scipy.linalg.lapack.dpotrf(np.array(A), lower=1)
    return int(info)


def first_bad_pivot(A):
    """Plain right-looking Cholesky that carries on as the GPU solver does: the first column whose pivot is not > 0 (NaN
    included), + 1; 0 if there is none."""
    W = np.tril(np.array(A, dtype=np.float64))
    first = 0
    with np.errstate(all="ignore"):
        for c in range(W.shape[0]):
            d = W[c, c]
            if not d > 0.0 and first == 0:
                first = c + 1
            col = W[c:, c] / np.sqrt(d)
            W[c:, c] = col
            W[c + 1:, c + 1:] -= np.tril(np.outer(col[1:], col[1:]))
    return first


def _two_product(a, b):
    """Dekker: a * b = p + e exactly, elementwise in f64 (no overflow or underflow at the magnitudes used here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_residual(A, b, parts):
    """b - A (sum of the f64 vectors `parts`), each row summed exactly (math.fsum over error-free products) and rounded
    once.  An np.longdouble residual has a floor of 2^-64 |A| |x|, only 2^-11 below f64's unit round-off: too coarse to
    certify a reference as a thousand times better than LAPACK."""
    import math
    terms = [np.asarray(b, dtype=np.float64)[:, None]]
    for x in parts:
        p, e = _two_product(A, np.asarray(x, dtype=np.float64)[None, :])
        terms += [-p, -e]
    T = np.concatenate(terms, axis=1)
    return np.array([math.fsum(row) for row in T])


def refined_solve(A, B, max_steps=8, exact=False):
    """cho_solve in f64, then iterative refinement until the residual stops shrinking.  The solution is an np.longdouble
    array; residuals are computed in np.longdouble, or (`exact`, B a vector) exactly on the unevaluated sum of the f64
    corrections, which are then returned as well: (x, parts)."""
    cf = scipy.linalg.cho_factor(A, lower=True)
    B = np.asarray(B, dtype=np.float64)
    Al, Bl = A.astype(LD), B.astype(LD)
    parts = [scipy.linalg.cho_solve(cf, B)]
    X = parts[0].astype(LD)
    resid = (lambda: exact_residual(A, B, parts)) if exact else (lambda: Bl - Al @ X)
    R = resid()
    best = np.abs(R).max()
    for _ in range(max_steps):
        d = scipy.linalg.cho_solve(cf, np.asarray(R, dtype=np.float64))
        parts.append(d)
        X_prev, X = X, X + d.astype(LD)
        Rn = resid()
        rn = np.abs(Rn).max()
        if not rn < best:
            parts.pop()
            X = X_prev
            break
        R, best = Rn, rn
    return (X, parts) if exact else X


def round_bits(x, bits):
    m, e = np.frexp(x)
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)


def degraded_solve(A, B, bits=24):
    """f64 Cholesky solve with every pivot reciprocal 1 / sqrt(d) rounded to `bits` bits: what the solver would compute if
    the correction step behind its approximate reciprocal square root were missing."""
    n = A.shape[0]
    W = np.tril(np.array(A, dtype=np.float64))
    inv = np.zeros(n)
    for c in range(n):
        inv[c] = round_bits(1.0 / np.sqrt(W[c, c]), bits)
        W[c:, c] *= inv[c]
        W[c + 1:, c + 1:] -= np.tril(np.outer(W[c + 1:, c], W[c + 1:, c]))
    Y = np.array(B, dtype=np.float64)
    for c in range(n):
        Y[c] *= inv[c]
        Y[c + 1:] -= W[c + 1:, c].reshape((-1,) + (1,) * (Y.ndim - 1)) * Y[c]
    for c in range(n - 1, -1, -1):
        Y[c] *= inv[c]
        Y[:c] -= W[c, :c].reshape((-1,) + (1,) * (Y.ndim - 1)) * Y[c]
    return Y


# ---------------------------------------------------------------------------------------------- error measures
class Equilibrated:
    """The symmetrically equilibrated system of A in np.longdouble."""

    def __init__(self, A):
        self.s = np.sqrt(np.diag(A).astype(LD))
        self.Ah = A.astype(LD) / self.s[:, None] / self.s[None, :]
        self.normA = float(np.abs(self.Ah).sum(1).max())

    def eta(self, B, X, R=None):
        """Normwise backward error of each column of X [N, k] (or of the vector X).  R: the residual B - A X of the
        unscaled system where the caller has it more exactly than np.longdouble gives it."""
        Xh = (np.asarray(X).astype(LD).T * self.s).T
        Bh = (np.asarray(B).astype(LD).T / self.s).T
        R = np.abs(Bh - self.Ah @ Xh) if R is None else np.abs((np.asarray(R).astype(LD).T / self.s).T)
        return np.asarray(R.max(0) / (LD(self.normA) * np.abs(Xh).max(0) + np.abs(Bh).max(0)), dtype=np.float64)

    def fwd(self, X, Xref):
        Xh = (np.asarray(X).astype(LD).T * self.s).T
        Rh = (np.asarray(Xref).astype(LD).T * self.s).T
        return np.asarray(np.abs(Xh - Rh).max(0) / np.abs(Rh).max(0), dtype=np.float64)


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------------------------------------- the cases, computed once
class System:
    """One system of the accuracy tests with everything the CPU can say about it."""

    def __init__(self, n, band, tau, where, decades):
        self.key = (n, band, tau, where, decades)
        self.n, self.band = n, band
        self.base = chain(n, band, tau, where)
        self.A = units(self.base, decades) if decades else self.base
        self.Sb = dense_to_band(self.A, band)
        rng = np.random.default_rng([1, n, band])
        self.B = rng.normal(size=(6 * n, N_RHS))          # column q = right-hand side q; the single solves take column 0
        self.eq = Equilibrated(self.A)
        self.X_lapack = lapack_solve(self.A, self.B)
        self.X_ref = refined_solve(self.A, self.B)
        self.eta_lapack = self.eq.eta(self.B, self.X_lapack)
        self.fwd_lapack = self.eq.fwd(self.X_lapack, self.X_ref)

    def certify(self, q):
        """Right-hand side q solved once more with exact residuals (two steps, which is enough to leave np.longdouble's
        resolution behind): (eta of that solve, forward distance of X_ref[:, q] from it)."""
        x, parts = refined_solve(self.A, self.B[:, q], max_steps=2, exact=True)
        eta = self.eq.eta(self.B[:, q], x, exact_residual(self.A, self.B[:, q], parts))
        return float(eta), float(self.eq.fwd(self.X_ref[:, q], x))

    @functools.cached_property
    def cond(self):
        return float(np.linalg.cond(self.A))

    def label(self):
        n, band, tau, where, d = self.key
        return f"({n},{band}) tau={tau:g} {where}" + (f" units({d})" if d else "")


@functools.lru_cache(maxsize=None)
def system(n, band, tau, where, decades=0):
    return System(n, band, tau, where, decades)


def accuracy_keys(shapes=SHAPES):
    return [(n, band, tau, where, d) for (n, band) in shapes for where in WHERES for tau in TAUS for d in (0, 3)]


# ---------------------------------------------------------------------------------------------- the shared assertions
def eta_bound(eta_lapack):
    return 8.0 * max(float(np.max(eta_lapack)), EPS)


def fwd_bound(fwd_lapack):
    return 16.0 * max(float(np.max(fwd_lapack)), 1e-15)


def check_accuracy(sysm, X, what=""):
    """X [N, k]: solutions of the first k right-hand sides of `sysm` by the solver under test.  Finite, with
    eta <= 8 max(eta_LAPACK of that system, 2^-52) and fwd <= 16 max(fwd_LAPACK over the system's right-hand sides, 1e-15).
    Returns (eta, fwd), the largest over the k columns."""
    X = np.asarray(X)
    assert np.isfinite(X).all(), (sysm.label(), what, "solution not finite")
    k = X.shape[1]
    eta = float(sysm.eq.eta(sysm.B[:, :k], X).max())
    fwd = float(sysm.eq.fwd(X, sysm.X_ref[:, :k]).max())
    assert eta <= eta_bound(sysm.eta_lapack), (sysm.label(), what, "eta", eta, "bound", eta_bound(sysm.eta_lapack))
    assert fwd <= fwd_bound(sysm.fwd_lapack), (sysm.label(), what, "fwd", fwd, "bound", fwd_bound(sysm.fwd_lapack))
    return eta, fwd


def check_status(status, c, exact, what=""):
    """A solve that met its first non-positive pivot in scalar column c: status == c + 1 where the elimination order is
    the one-sided one (`exact`), some column + 1 > 0 otherwise; never 0."""
    if exact:
        assert status == c + 1, (what, "status", status, "expected", c + 1)
    else:
        assert status > 0, (what, "status", status, "column", c)


# ---------------------------------------------------------------------------------------------- selected inversion
def inverse_ref(A):
    """A^-1, dense in np.longdouble, from refined solves of the identity columns."""
    return refined_solve(A, np.eye(A.shape[0]))


def selinv_error(Sg, Sigma_ref, band):
    """Largest entrywise |Sigma_ij - Sigma_ref,ij| / sqrt(Sigma_ref,ii Sigma_ref,jj) over the stored band."""
    S = band_to_dense(np.asarray(Sg, dtype=np.float64)).astype(LD)
    n = S.shape[0] // 6
    d = np.sqrt(np.diag(Sigma_ref))
    E = np.abs(S - Sigma_ref) / d[:, None] / d[None, :]
    blk = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) <= band
    return float((E * np.kron(blk, np.ones((6, 6)))).max())
