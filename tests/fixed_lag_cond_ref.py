"""CPU reference for the numerics of fixed-lag marginalisation (tests/test_fixed_lag_cond_ref.py,
tests/test_fixed_lag_cond_gpu.py): seeded families of ill-conditioned, badly scaled and gauge-free block bands whose head is
marginalised, a refined np.longdouble Schur complement, componentwise error measures, the sliding-window recursion of the
smoother at kernel level, and the assertions both test files share.  Test infrastructure only: numpy and scipy.

It sits on band_cond_ref.py (chain, units, pow4, with_nan, indefinite, first_bad_pivot, refined_solve) and on fixed_lag_ref.py,
whose marginal / marginal_head are "the f64 numpy statement": every bound below is a ratio over what that statement reaches
on the same system.

  free_chain(n, band)           the factors of band_cond_ref.chain without any prior: the exact 6-dimensional gauge null space
  marginal_ref(A, b, n_drop)    H, g, quad in np.longdouble with the magnitude sums the errors are measured against
  cw_err(got, ref, mag)         max |got - ref| / mag over mag > 0; an entry with mag == 0 must be exactly 0 (else inf)
  Recursion(T, band, tau, d)    step t assembles the factors whose lower node is dropped at step t onto the prior of step
                                t - 1, drops n_drop nodes, passes (H, g) on and accumulates c; its reference is the ONE-SHOT
                                marginal of all those factors by marginal_ref on the whole dense matrix
  panel_marginal(...)           the kernel's arithmetic in numpy (48-column panels on a dense lower triangle with the gradient
                                as one more row), with switches for the deliberately wrong variants the CPU test rejects"""
import functools
from collections import namedtuple

import numpy as np
import scipy.linalg

import band_cond_ref as bc
import fixed_lag_ref as fl
from marginals_ref import dense_to_band

LD = bc.LD
EPS = bc.EPS
PW = 48                       # columns of a panel of the kernel (8 nodes)
FACTOR, FLOOR = 16.0, 1e-15   # the project's ratio and floor (band_cond_ref.fwd_bound, the selected-inversion bound)

# (n, band, n_drop): n - n_drop <= band + 1
SHAPES = ((9, 2, 6), (23, 7, 15), (23, 7, 16), (23, 7, 17), (40, 30, 9), (40, 30, 33), (64, 20, 45), (64, 20, 48), (131, 37, 93))
POW4_SHAPES = ((23, 7, 17), (64, 20, 45))
# (tau, where); tau None: free_chain
FAMILIES = tuple((tau, where) for where in bc.WHERES for tau in bc.TAUS) + ((None, None),)
# (T, band, tau, decades) of the recursion; the prior tau I sits on node 0 only (tau = 0: none, the chain is gauge-free)
RECURSIONS = ((150, 5, 1e-2, 0), (150, 5, 1e-8, 3), (150, 5, 0.0, 0), (150, 5, 0.0, 3), (120, 12, 1e-8, 3), (120, 12, 0.0, 3))
# the variant with velocity padding: 3 nodes per step, the kept part is two whole keyframes
PADDED_RECURSION = (40, 6, 1e-5, 3)


# ---------------------------------------------------------------------------------------------- families
def chain_factors(n, band, key, padded=False):
    """The pair factors of band_cond_ref.chain as (i, k, M), i > k >= i - band, M = sym(J^T J) in np.longdouble with
    J = I + 0.3 N(0, 1): the pair i - k = 1 always, the others with probability 1/2.  The factor adds M to the blocks (i, i)
    and (k, k) and -M to (i, k) and (k, i).  `padded`: returns (i, k, Mii, Mkk, Mik) instead, with the last three coordinates
    of every node 3 q + 1 (a velocity node's padding) projected out of the factor."""
    rng = np.random.default_rng([7, n, band, *key])
    out = []
    for i in range(1, n):
        for k in range(max(0, i - band), i):
            Ji = (np.eye(6) + 0.3 * rng.normal(size=(6, 6))).astype(LD)
            if not ((i - k == 1) or rng.random() < 0.5):
                continue
            M = Ji.T @ Ji
            M = 0.5 * (M + M.T)
            if padded:
                Pi, Pk = (np.diag(np.r_[np.ones(3), np.zeros(3) if q % 3 == 1 else np.ones(3)]).astype(LD) for q in (i, k))
                out.append((i, k, Pi @ M @ Pi, Pk @ M @ Pk, Pi @ M @ Pk))
            else:
                out.append((i, k, M))
    return out


def free_chain(n, band):
    """band_cond_ref.chain without a prior: positive semi-definite with the exact null space x_i all equal.  Accumulated
    in np.longdouble and rounded once."""
    A = np.zeros((6 * n, 6 * n), dtype=LD)
    for i, k, M in chain_factors(n, band, (0,)):
        si, sk = slice(6 * i, 6 * i + 6), slice(6 * k, 6 * k + 6)
        A[si, si] += M
        A[sk, sk] += M
        A[si, sk] -= M
        A[sk, si] -= M
    return np.asarray(A, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def base_matrix(n, band, tau, where):
    return free_chain(n, band) if tau is None else bc.chain(n, band, tau, where)


# ---------------------------------------------------------------------------------------------- the reference
Ref = namedtuple("Ref", "H g quad magH magg magq")


def _solve_ld(S, B):
    """S X = B with S, B in np.longdouble: band_cond_ref.refined_solve on the rounded system, then refinement against the
    unrounded one (the two differ only where S is not an array of f64 values)."""
    S64, B64 = np.asarray(S, dtype=np.float64), np.asarray(B, dtype=np.float64)
    X = bc.refined_solve(S64, B64)
    if np.array_equal(S64.astype(LD), S) and np.array_equal(B64.astype(LD), B):
        return X
    cf = scipy.linalg.cho_factor(S64, lower=True)
    for _ in range(3):
        X = X + scipy.linalg.cho_solve(cf, np.asarray(B - S @ X, dtype=np.float64)).astype(LD)
    return X


def marginal_ref(A, b, n_drop):
    """The marginal of the first n_drop nodes in np.longdouble (A f64 or np.longdouble): X = S_MM^-1 [S_MR, g_M] refined,
    H = S_RR - S_RM X, g = g_R - S_RM x_g, quad = g_M^T x_g, and magH = |S_RR| + |S_RM| |X|, magg = |g_R| + |S_RM| |x_g|,
    magq = |g_M|^T |x_g|."""
    K = 6 * n_drop
    Al, bl = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    SMM, SRM, SRR = Al[:K, :K], Al[K:, :K], Al[K:, K:]
    X = _solve_ld(SMM, np.column_stack([SRM.T, bl[:K]]))
    XH, xg = X[:, :-1], X[:, -1]
    H = SRR - SRM @ XH
    magH = np.abs(SRR) + np.abs(SRM) @ np.abs(XH)
    return Ref(0.5 * (H + H.T), bl[K:] - SRM @ xg, bl[:K] @ xg, 0.5 * (magH + magH.T), np.abs(bl[K:]) + np.abs(SRM) @ np.abs(xg),
               np.abs(bl[:K]) @ np.abs(xg))


def cw_err(got, ref, mag):
    """max |got - ref| / mag over the entries with mag > 0; an entry with mag == 0 must be exactly 0: inf if it is not."""
    got, ref, mag = (np.atleast_1d(np.asarray(x, dtype=LD)) for x in (got, ref, mag))
    zero = mag == 0
    if (got[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / mag[~zero]).max())


def errors(got, ref):
    """(errH, errg, errq) of got = (H, g, quad) against a Ref."""
    return cw_err(got[0], ref.H, ref.magH), cw_err(got[1], ref.g, ref.magg), cw_err(got[2], ref.quad, ref.magq)


def bound(e_numpy, factor=FACTOR):
    return factor * max(e_numpy, FLOOR)


def numpy_marginal(A, b, n_drop):
    """The f64 numpy statement as (H, g, quad, status): fixed_lag_ref.marginal_head with the Cholesky of S_MM."""
    H, g, c = fl.marginal_head(A, b, 0.0, n_drop, solve="cholesky")
    return H, g, -2.0 * c, 0


def lam_min(H, diag_RR):
    """The smallest eigenvalue of D^-1/2 H D^-1/2, D = diag S_RR with zero diagonals replaced by 1."""
    s = np.sqrt(np.where(np.asarray(diag_RR) > 0, diag_RR, 1.0).astype(LD))
    E = np.asarray(np.asarray(H, dtype=LD) / s[:, None] / s[None, :], dtype=np.float64)
    return float(np.linalg.eigvalsh(0.5 * (E + E.T))[0])


def psd_bound(lam_numpy, rows, factor=FACTOR):
    """lambda_min >= -factor max(-lambda_min of the numpy statement, rows 2^-52), rows = 6 w."""
    return -factor * max(-lam_numpy, rows * EPS)


def null_err(H):
    """max |H Z| / (|H| |Z|), Z the stacked 6 x 6 identities (the gauge directions of a chain; units() scales its columns
    only).  A row whose |H| |Z| is 0 must give exactly 0."""
    Hl = np.asarray(H, dtype=LD)
    Z = np.tile(np.eye(6, dtype=LD), (Hl.shape[0] // 6, 1))
    return cw_err(Hl @ Z, np.zeros((Hl.shape[0], 6)), np.abs(Hl) @ Z)


# ---------------------------------------------------------------------------------------------- the systems, computed once
class MSystem:
    """One system of the accuracy tests with everything the CPU can say about it."""

    def __init__(self, n, band, n_drop, tau, where, decades):
        assert n - n_drop <= band + 1
        self.key = (n, band, n_drop, tau, where, decades)
        self.n, self.band, self.n_drop, self.free = n, band, n_drop, tau is None
        base = base_matrix(n, band, tau, where)
        self.A = bc.units(base, decades) if decades else base
        self.b = np.random.default_rng([2, n, band, n_drop]).normal(size=6 * n) * np.abs(self.A).max()
        self.Sb = dense_to_band(self.A, band)
        self.K = 6 * n_drop
        self.diag_RR = np.diag(self.A)[self.K:].copy()

    @functools.cached_property
    def ref(self):
        return marginal_ref(self.A, self.b, self.n_drop)

    @functools.cached_property
    def numpy(self):
        return numpy_marginal(self.A, self.b, self.n_drop)

    @functools.cached_property
    def err_numpy(self):
        return errors(self.numpy, self.ref)

    @functools.cached_property
    def lam_numpy(self):
        return lam_min(self.numpy[0], self.diag_RR)

    @functools.cached_property
    def null_numpy(self):
        return null_err(self.numpy[0])

    @functools.cached_property
    def cond(self):
        return float(np.linalg.cond(self.A[:self.K, :self.K]))

    def label(self):
        return label_of(self.key)


def label_of(key):
    n, band, k, tau, where, d = key
    fam = "free" if tau is None else f"tau={tau:g} {where}"
    return f"({n},{band},{k}) {fam}" + (f" units({d})" if d else "")


@functools.lru_cache(maxsize=None)
def system(n, band, n_drop, tau, where, decades=0):
    return MSystem(n, band, n_drop, tau, where, decades)


def accuracy_keys(shapes=SHAPES):
    return [(n, band, k, tau, where, d) for (n, band, k) in shapes for (tau, where) in FAMILIES for d in (0, 3)]


# ---------------------------------------------------------------------------------------------- the shared assertions
def check_marginal(got, sysm, factor=FACTOR, what=""):
    """got = (H, g, quad) of the marginalisation under test: finite, H bit-symmetric, and each of errH, errg, errq at most
    factor max(the same measure of the numpy statement on that system, 1e-15).  Returns (errH, errg, errq)."""
    H, g, quad = np.asarray(got[0]), np.asarray(got[1]), float(got[2])
    assert np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(quad), (sysm.label(), what, "result not finite")
    assert np.array_equal(H, H.T), (sysm.label(), what, "H is not bit-symmetric")
    e = errors((H, g, quad), sysm.ref)
    for name, got_e, np_e in zip(("errH", "errg", "errq"), e, sysm.err_numpy):
        assert got_e <= bound(np_e, factor), (sysm.label(), what, name, got_e, "bound", bound(np_e, factor))
    return e


def check_psd(H, sysm, factor=FACTOR, what=""):
    lam = lam_min(H, sysm.diag_RR)
    lo = psd_bound(sysm.lam_numpy, len(sysm.diag_RR), factor)
    assert lam >= lo, (sysm.label(), what, "lambda_min", lam, "bound", lo)
    return lam


def check_null(H, sysm, factor=FACTOR, what=""):
    e = null_err(H)
    assert e <= bound(sysm.null_numpy, factor), (sysm.label(), what, "null space", e, "bound", bound(sysm.null_numpy, factor))
    return e


def expected_status(c, K):
    """The status of a system whose first bad pivot is scalar column c: c + 1 inside S_MM (c < K), 0 in the kept part, which
    the marginalisation does not factor."""
    return c + 1 if c < K else 0


def check_status(status, c, K, what=""):
    assert status == expected_status(c, K), (what, "status", status, "expected", expected_status(c, K), "column", c, "K", K)


def cpu_status(A, n_drop):
    """What the CPU says the status of marginalising A's first n_drop nodes is: band_cond_ref.first_bad_pivot of S_MM."""
    return bc.first_bad_pivot(np.asarray(A)[:6 * n_drop, :6 * n_drop])


def status_columns(N, K):
    """The scalar columns of the status tests: every column of panels 0 and 1, the first and last column of every later
    panel, the last column K - 1 of the (partial) last panel -- and K and N - 1, the first and last column of the kept part."""
    cols = set(range(min(2 * PW, K)))
    for c0 in range(2 * PW, K, PW):
        cols |= {c0, min(c0 + PW, K) - 1}
    return sorted(cols | {K - 1, K, N - 1})


def nan_entries(n, band, n_drop):
    """band_cond_ref.nan_positions inside the dropped part (r < K), inside the kept part (r, c >= K) and one entry of S_RM
    (r >= K > c): sub-diagonal scalar entries (r, c) inside the band."""
    K = 6 * n_drop
    p = n_drop // 2
    q = min(n_drop - 1, p + band)
    head = [(6 * p + 4, 6 * p + 1), (6 * q + 2, 6 * p + 3)]
    w = n - n_drop
    p = n_drop + w // 2
    tail = [(6 * p + 4, 6 * p + 1), (6 * (n - 1) + 2, 6 * p + 3), (K + 2, K - 3)]
    return head, tail


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic
def panel_marginal(A, b, n_drop, **switches):
    """_panel_marginal with floating-point warnings off: behind a bad pivot the numbers mean nothing, as in the kernel."""
    with np.errstate(all="ignore"):
        return _panel_marginal(A, b, n_drop, **switches)


def _panel_marginal(A, b, n_drop, inv_bits=None, skip_partial=False, skip_gradient=False, stale_triangle=False):
    """(H, g, quad, status) by the arithmetic of vus_ba_band_marginalize in f64 numpy: the lower triangle of A with b as row
    N, per 48-column panel the factor of the diagonal block, the rows below solved against it, the outer product subtracted
    from the trailing lower triangle; H mirrored from the lower triangle.  The switches make it wrong on purpose:
      inv_bits        every pivot reciprocal 1 / sqrt(d) rounded to that many bits (band_cond_ref.degraded_solve)
      skip_partial    only whole panels are eliminated, the last, partial one is skipped
      skip_gradient   the trailing update leaves the gradient row out
      stale_triangle  H is mirrored from the UPPER triangle of the work matrix, which no update touches"""
    N, K = A.shape[0], 6 * n_drop
    T = np.zeros((N + 1, N + 1))
    T[:N, :N] = A if stale_triangle else np.tril(A)
    T[N, :N] = b
    status = 0
    for c0 in range(0, K, PW):
        pw = min(PW, K - c0)
        if skip_partial and pw < PW:
            break
        for c in range(c0, c0 + pw):
            d = T[c, c]
            if not d > 0.0:
                status = status or c + 1
                d = 1.0
            if inv_bits is None:
                T[c, c] = np.sqrt(d)
                T[c + 1:, c] /= T[c, c]
            else:
                inv = bc.round_bits(1.0 / np.sqrt(d), inv_bits)
                T[c, c] = d * inv
                T[c + 1:, c] *= inv
            last = N if skip_gradient else N + 1
            col = T[c + 1:last, c]
            T[c + 1:last, c + 1:last] -= np.tril(np.outer(col, col))
    L = T[K:N, K:N]
    H = (np.triu(L) + np.triu(L, 1).T) if stale_triangle else (np.tril(L) + np.tril(L, -1).T)
    return H, T[N, K:N].copy(), -T[N, N], status


# ---------------------------------------------------------------------------------------------- the recursion
class Recursion:
    """The sliding-window arithmetic of the smoother at kernel level over the chain of n = n_drop T + band nodes with the
    prior tau I on node 0 (tau = 0: none) and units(., decades).  Step t takes the band + n_drop nodes from n_drop t on,
    assembles every chain factor whose lower node it drops (each factor rounded to f64 once, then plain f64 additions in a
    fixed order), the prior of step t - 1 on the first `band` nodes and a random gradient on the dropped nodes, drops
    n_drop nodes, passes (H, g) on and accumulates c = -quad / 2.  `padded` (n_drop = 3, band a multiple of 3): nodes
    3 q + 1 are velocity nodes whose last three coordinates carry nothing but a unit diagonal."""

    def __init__(self, T, band, tau, decades, n_drop=1, padded=False):
        assert not padded or (n_drop == 3 and band % 3 == 0)
        self.key = (T, band, tau, decades, n_drop, padded)
        self.T, self.band, self.tau, self.n_drop, self.padded = T, band, tau, n_drop, padded
        self.w = band + n_drop                             # nodes of a step's system
        self.n = n = n_drop * T + band
        d6 = np.concatenate([np.ones(3, LD), np.full(3, LD(10) ** -decades)])
        D = np.outer(d6, d6)
        r = lambda M: np.asarray(D * M, dtype=np.float64)
        self.by_lower = [[] for _ in range(n)]
        for f in chain_factors(n, band, (int(T), int(decades), int(padded)), padded):
            i, k = f[0], f[1]
            Mii, Mkk, Mik = (f[2], f[2], f[2]) if not padded else f[2:]
            self.by_lower[k].append((i, r(Mii), r(Mkk), r(Mik)))
        self.anchor = r(LD(tau) * np.eye(6, dtype=LD))
        rng = np.random.default_rng([8, T, band, int(decades), n_drop])
        self.grad = np.asarray(d6, dtype=np.float64) * rng.normal(size=(n, 6))
        self.pad = np.array([6 * q + c for q in range(n) if q % 3 == 1 for c in (3, 4, 5)], dtype=np.int64) if padded else None
        if padded:
            self.grad.reshape(-1)[self.pad] = 0.0

    def label(self):
        T, band, tau, d, k, padded = self.key
        return f"T={T} band={band} tau={tau:g}" + (f" units({d})" if d else "") + (f" drop {k} padded" if padded else "")

    def _add(self, A, b, lo, nodes):
        """Adds the factors whose lower node is in `nodes` (and the anchor, the gradients) to A, b whose node 0 is `lo`."""
        for k in nodes:
            sk = slice(6 * (k - lo), 6 * (k - lo) + 6)
            if k == 0 and self.tau:
                A[sk, sk] += self.anchor
            b[sk] += self.grad[k]
            for i, Mii, Mkk, Mik in self.by_lower[k]:
                si = slice(6 * (i - lo), 6 * (i - lo) + 6)
                A[si, si] += Mii
                A[sk, sk] += Mkk
                A[si, sk] -= Mik
                A[sk, si] -= Mik.T
        if self.padded:
            p = self.pad[(self.pad >= 6 * lo) & (self.pad < 6 * lo + A.shape[0])] - 6 * lo
            A[p, p] = 1.0

    def step_system(self, t, prior):
        """The dense f64 system (A, b) of step t over its band + n_drop nodes; prior = (H, g) of step t - 1 or None."""
        m = 6 * self.w
        A, b = np.zeros((m, m)), np.zeros(m)
        if prior is not None:
            A[:6 * self.band, :6 * self.band] += prior[0]
            b[:6 * self.band] += prior[1]
        lo = self.n_drop * t
        self._add(A, b, lo, range(lo, lo + self.n_drop))
        return A, b

    def run(self, marginalize, each=None):
        """marginalize(A, b, n_drop) -> (H, g, quad, status) at every step; each(t, A, b, H, g, status) after it.  Returns
        (H, g, quad accumulated): c = -quad / 2."""
        prior, quad = None, 0.0
        for t in range(self.T):
            A, b = self.step_system(t, prior)
            H, g, q, status = marginalize(A, b, self.n_drop)
            if each is not None:
                each(t, A, b, H, g, status)
            prior, quad = (H, g), quad + q
        return prior[0], prior[1], quad

    @functools.cached_property
    def one_shot(self):
        """The one-shot marginal of every factor with a dropped lower node onto the last `band` nodes: marginal_ref on the
        whole dense matrix, the sum of the same f64 factors in np.longdouble, not rounded."""
        m = 6 * self.n
        A, b = np.zeros((m, m), dtype=LD), np.zeros(m, dtype=LD)
        self._add(A, b, 0, range(self.n_drop * self.T))
        self.diag_RR = np.asarray(np.diag(A)[-6 * self.band:], dtype=np.float64)
        self.cond = float(np.linalg.cond(np.asarray(A[:-6 * self.band, :-6 * self.band], dtype=np.float64)))
        return marginal_ref(A, b, self.n_drop * self.T)

    @functools.cached_property
    def numpy(self):
        """The recursion by the numpy statement: (H, g, quad), its errors against the one-shot reference, lambda_min, and
        the null-space measure."""
        H, g, quad = self.run(numpy_marginal)
        ref = self.one_shot
        return dict(H=H, g=g, quad=quad, err=errors((H, g, quad), ref), lam=lam_min(H, self.diag_RR), null=null_err(H))

    def check(self, got, factor=FACTOR, what=""):
        """got = (H, g, quad) after T steps: errH, errg and the accumulated constant against the one-shot reference at most
        factor max(the numpy recursion's, 1e-15); the PSD bound; for tau = 0 the null-space bound.  Returns the figures."""
        H, g, quad = got
        ref, ny = self.one_shot, self.numpy
        assert np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(quad), (self.label(), what, "not finite")
        e = errors(got, ref)
        for name, got_e, np_e in zip(("errH", "errg", "errq"), e, ny["err"]):
            assert got_e <= bound(np_e, factor), (self.label(), what, name, got_e, "bound", bound(np_e, factor))
        lam = lam_min(H, self.diag_RR)
        assert lam >= psd_bound(ny["lam"], 6 * self.band, factor), (self.label(), what, "lambda_min", lam)
        ne = null_err(H) if self.tau == 0 and not self.padded else None
        if ne is not None:
            assert ne <= bound(ny["null"], factor), (self.label(), what, "null space", ne, "bound", bound(ny["null"], factor))
        return e, lam, ne


@functools.lru_cache(maxsize=None)
def recursion(T, band, tau, decades, n_drop=1, padded=False):
    return Recursion(T, band, tau, decades, n_drop, padded)


def check_prior(H, g, what=""):
    """What vus_window_prior_check enforces of (H, g): finite, diagonal >= 0, asymmetry <= 1e-12 hmax."""
    assert np.isfinite(H).all() and np.isfinite(g).all(), (what, "not finite")
    assert (np.diag(H) >= 0.0).all(), (what, "negative diagonal", float(np.diag(H).min()))
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max(), (what, "not symmetric")


# ---------------------------------------------------------------------------------------------- priors for the family tests
PRIOR_KINDS = ("plain", "units", "free")


@functools.lru_cache(maxsize=None)
def prior_of(rows, kind):
    """(H [rows, rows], g, c): the leading principal part of a numpy-statement marginal of matching size -- of
    chain(tau = 1e-2 on every pose) plain or under units(., 3), or of free_chain (positive semi-definite; before the cut,
    gauge-free) -- nine dropped nodes in front of w = ceil(rows / 6) kept ones, band w."""
    w = -(-rows // 6)
    n = w + 9
    base = free_chain(n, w) if kind == "free" else bc.chain(n, w, 1e-2, "all")
    A = bc.units(base, 3) if kind == "units" else base
    b = np.random.default_rng([3, rows]).normal(size=6 * n) * np.abs(A).max()
    H, g, c = fl.marginal_head(A, b, 0.37, 9)
    return np.ascontiguousarray(H[:rows, :rows]), g[:rows].copy(), float(c)


def prior_energy_ref(H, g, c, u):
    """(g + H u, c + g^T u + u^T H u / 2, the magnitudes |g| + |H| |u| and |c| + |g|^T |u| + |u|^T |H| |u| / 2) in
    np.longdouble."""
    Hl, gl, ul = (np.asarray(x, dtype=LD) for x in (H, g, u))
    Hu, aHu = Hl @ ul, np.abs(Hl) @ np.abs(ul)
    return (gl + Hu, LD(c) + gl @ ul + 0.5 * (ul @ Hu), np.abs(gl) + aHu, abs(LD(c)) + np.abs(gl) @ np.abs(ul) + 0.5 * (np.abs(ul) @ aHu))


def nav_padding_masks(nN, band):
    """Boolean masks of the entries of Sband [nN, band + 1, 36] and gs [nN, 6] that belong to a velocity node's padding."""
    S, g = np.zeros((nN, band + 1, 6, 6), bool), np.zeros((nN, 6), bool)
    g[1::3, 3:] = True
    for q in range(nN):
        for sl in range(min(q, band) + 1):
            if q % 3 == 1:
                S[q, sl, 3:, :] = True
            if (q - sl) % 3 == 1:
                S[q, sl, :, 3:] = True
    return S.reshape(nN, band + 1, 36), g
