"""CPU harness for the long-closure low-rank solve on ill-conditioned systems (tests/test_closure_cond_ref.py certifies it,
tests/test_closure_cond_gpu.py holds vus_ba_band_resolve and the vus_closure_* stages to it).  Test infrastructure only:
numpy (and scipy through band_cond_ref).  Built from band_cond_ref (the band families, the refined reference, the
equilibrated error measures and their bounds) and closure_ref (the layout of the stored factor, U, C and the low-rank solve).

A system is A = B + U U^T:
  B       band_cond_ref.system(n, band, tau, where, decades): chain, and units(chain, 3), for tau in TAUS, both WHERES
  U       [6 n, 6 k], closure_ref.u_matrix of k synthetic factors [J1 | J2] on two nodes more than `band` apart; J2 a random
          upper-triangular matrix with condition <= 10 (what `rows` holds under sqrt_info), J1 = -J2: a relative measurement
          of the chain family (random_factors says why, and what an independent J1 does); LAYOUTS names the k factors
  gamma   max |U U^T| / max |B|, set by scaling the rows
  stride  pose_stride: the factors sit on nodes stride * pose
The keys of keys(): every (shape, B, gamma) that is admissible() -- A is still a system of f64 -- once, with the layout
walking through LAYOUTS from key to key; plus pose_stride 2 on (40,30) and 3 on (57,1).  The full cross with the layouts
as well would be 960 dense systems of up to 786 unknowns.

The bridge family (an odometry dropout that a closure bridges): chain(n, band, 1e-2, "first") whose factors across the
cut n / 2 are weighted by beta (their whole J^T J: diagonal and off-diagonal blocks), plus lambda I, plus one closure, or
three, across the cut at gamma = 1.

Per system, on the 7 right-hand sides of the band system:  X_ref (refined), X_direct (LAPACK Cholesky on A: the widened
band), X_wood (closure_ref.lowrank_solve in f64: the algorithm the kernels run), eta and fwd of both from Equilibrated(A).
A candidate X passes check() with eta <= eta_bound(max(eta_wood, eta_direct)) and fwd <= fwd_bound(max(fwd_wood, fwd_direct)).
A system is of the ACCURACY family if fwd_wood <= 64 max(fwd_direct, 1e-15), else of the LOSS family: the low-rank
algorithm itself loses digits there that the widened band keeps."""
import functools

import numpy as np

import band_cond_ref as bc
import closure_ref as cr

LD = bc.LD
SHAPES = ((23, 7), (57, 1), (40, 30), (131, 37))
GAMMAS = (1e-6, 1.0, 1e6, 1e12)
LAYOUTS = ("one", "seven", "k63", "k64", "same64")
STRIDE_KEYS = {2: (40, 30), 3: (57, 1)}           # pose_stride -> the shape it is exercised on
FAMILY_RATIO, FAMILY_FLOOR = 64.0, 1e-15
BETAS = (1.0, 1e-4, 1e-8, 1e-12, 0.0)
LAMBDAS = (1e-3, 1e-7, 1e-11)
BRIDGE_SHAPES = ((23, 7), (57, 1))
BRIDGE_CLOSURES = (1, 3)


# ---------------------------------------------------------------------------------------------- the factors
def layout_pairs(layout, n_poses, min_span):
    """Pose pairs (i, j) of a layout: every |i - j| >= min_span (the first pose distance outside the band)."""
    D, last = min_span, n_poses - 1
    r = n_poses - D                                   # poses that can start a closure
    assert r >= 3, (n_poses, min_span)
    if layout == "one":
        return [(r // 2, r // 2 + D)]
    if layout == "seven":      # exactly min_span apart; two on one pair; both key orders; (0, .) three times: shared nodes
        return [(0, D), (1, last - 1), (1, last - 1), (last, 2), (0, last), (last - 1, 0), (2, last)]
    if layout == "same64":
        return [(r // 2, r // 2 + D)] * 64
    k = {"k63": 63, "k64": 64}[layout]
    out = []
    for f in range(k):
        i = f % r
        j = i + D + (f // r) % (n_poses - D - i)
        out.append((i, j) if f % 2 == 0 else (j, i))
    return out


def random_factors(rng, pairs, relative=True):
    """closure_ref-style factor tuples (r, J1, J2, i, j, None, None), r = 0.  J2 = R, the upper-triangular factor of
    Q1 diag(s) Q2^T with s in [1, 10] (its singular values: condition <= 10).  `relative`: J1 = -R, a between factor of the
    chain family, whose factors are [J, -J]: it measures a relative pose and leaves the chain's gauge (the same motion of
    every pose) as free as the band system has it.  Otherwise J1 is a second, independent matrix of that kind, not
    triangular: such a factor also holds the gauge, which no relative measurement does."""
    def cond10():
        Q1, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        Q2, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        return (Q1 * 10.0 ** rng.uniform(0.0, 1.0, 6)) @ Q2.T
    fac = []
    for i, j in pairs:
        J2 = np.triu(np.linalg.qr(cond10())[1])
        J1 = -J2 if relative else cond10()
        fac.append((np.zeros(6), J1, J2, int(i), int(j), None, None))
    return fac


def scaled(fac, s):
    return [(r, s * J1, s * J2, i, j, a, b) for r, J1, J2, i, j, a, b in fac]


def low_rank_term(U):
    """U U^T in np.longdouble, factor by factor: a factor's six columns are non-zero on the rows of its two nodes only."""
    out = np.zeros((U.shape[0], U.shape[0]), dtype=LD)
    for c in range(0, U.shape[1], 6):
        idx = np.nonzero(U[:, c:c + 6].any(1))[0]
        V = U[idx, c:c + 6].astype(LD)
        out[np.ix_(idx, idx)] += V @ V.T
    return out


# ---------------------------------------------------------------------------------------------- the low-rank solve and its defects
def lowrank(B, U, b, z_bits=None, identity=True, upper=False, flip=None, U_alg=None):
    """closure_ref.lowrank_solve(B, U, b), or one of the defective forms the harness must catch:
      z_bits    Z rounded to that many bits
      identity  False: C = U^T Z, without its + I
      upper     C factored from its UPPER triangle after the entry (0, 1) of it moved by 1e-9 sqrt(C_00 C_11)
      flip      the correction ADDED on right-hand side `flip`
      U_alg     the U the algorithm sees (A keeps the whole U)"""
    if z_bits is None and identity and not upper and flip is None and U_alg is None:
        return cr.lowrank_solve(B, U, b)
    U = U if U_alg is None else U_alg
    x0 = np.linalg.solve(B, b)
    Z, C = cr.capacitance(B, U)
    if z_bits is not None:
        Z = bc.round_bits(Z, z_bits)
        C = np.eye(U.shape[1]) + U.T @ Z
    if not identity:
        C = C - np.eye(U.shape[1])
    if upper:
        C = C.copy()
        C[0, 1] += 1e-9 * np.sqrt(C[0, 0] * C[1, 1])
        C = np.triu(C) + np.triu(C, 1).T
    with np.errstate(all="ignore"):
        try:
            corr = Z @ np.linalg.solve(C, U.T @ x0)
        except np.linalg.LinAlgError:
            corr = np.full_like(x0, np.nan)
    sign = np.ones(b.shape[1])
    if flip is not None:
        sign[flip] = -1.0
    return x0 - corr * sign


DEFECTS = {"Z at 24 bits": dict(z_bits=24), "C without + I": dict(identity=False), "C from its perturbed upper triangle": dict(upper=True),
           "correction added on one right-hand side": dict(flip=3), "U without the last J2": None}


# ---------------------------------------------------------------------------------------------- the systems, computed once
_FAMILY = {}      # name -> (accurate, loss ratio, fwd_wood, fwd_direct) of every system built so far: system() keeps only the last 48


class ClosureSystem:
    """B, the factors, A = B + U U^T and everything the CPU can say about it."""

    def __init__(self, name, Bm, band, fac, stride, rhs):
        self.name, self.band, self.stride = name, band, stride
        self.n = Bm.shape[0] // 6
        self.Bm, self.Sb, self.fac = Bm, bc.dense_to_band(Bm, band), fac
        self.k, self.m = len(fac), 6 * len(fac)
        self.rows = cr.rows(fac)
        self.rows[:, 72:] = 0.0
        self.U = cr.u_matrix(fac, self.n, stride)
        self.pairs = [(f[3], f[4]) for f in fac]
        assert all(stride * abs(i - j) > band for i, j in self.pairs)
        self.A = np.asarray(Bm.astype(LD) + low_rank_term(self.U), dtype=np.float64)
        self.B = rhs                                  # [N, 7]: column q = right-hand side q
        self.factored = bc.lapack_status(self.A) == 0      # False: A is not positive definite in f64, nothing below exists
        if not self.factored:
            return
        self.eq = bc.Equilibrated(self.A)
        self.X_ref = bc.refined_solve(self.A, rhs)
        self.X_direct = bc.lapack_solve(self.A, rhs)
        self.X_wood = lowrank(Bm, self.U, rhs)
        self.eta_direct, self.fwd_direct = self.eq.eta(rhs, self.X_direct), self.eq.fwd(self.X_direct, self.X_ref)
        self.eta_wood, self.fwd_wood = self.eq.eta(rhs, self.X_wood), self.eq.fwd(self.X_wood, self.X_ref)
        _FAMILY[name] = (self.accurate, self.loss_ratio, float(self.fwd_wood.max()), float(self.fwd_direct.max()))

    # -- the bounds and the family
    @property
    def eta_bound(self):
        return bc.eta_bound(max(self.eta_wood.max(), self.eta_direct.max()))

    @property
    def fwd_bound(self):
        return bc.fwd_bound(max(self.fwd_wood.max(), self.fwd_direct.max()))

    @property
    def loss_ratio(self):
        return float(self.fwd_wood.max() / max(self.fwd_direct.max(), FAMILY_FLOOR))

    @property
    def accurate(self):
        """Member of the accuracy family: the low-rank algorithm in f64 LAPACK keeps the widened band's digits here."""
        return self.loss_ratio <= FAMILY_RATIO

    def measure(self, X, cols=None):
        """(finite, eta, fwd) of the candidate X [N, k] for right-hand sides `cols` (default: the first k), the largest
        over the columns; NaN where X is not finite."""
        X = np.asarray(X)
        cols = list(range(X.shape[1])) if cols is None else list(cols)
        if not np.isfinite(X).all():
            return False, np.nan, np.nan
        return True, float(self.eq.eta(self.B[:, cols], X).max()), float(self.eq.fwd(X, self.X_ref[:, cols]).max())

    def check(self, X, what="", cols=None):
        finite, eta, fwd = self.measure(X, cols)
        assert finite, (self.name, what, "solution not finite")
        assert eta <= self.eta_bound, (self.name, what, "eta", eta, "bound", self.eta_bound)
        assert fwd <= self.fwd_bound, (self.name, what, "fwd", fwd, "bound", self.fwd_bound)
        return eta, fwd

    def passes(self, X):
        try:
            self.check(X)
        except AssertionError:
            return False
        return True

    def defective(self, which):
        """X of the low-rank solve with the defect DEFECTS names."""
        kw = DEFECTS[which]
        if kw is None:
            U_alg = self.U.copy()
            b = self.stride * self.pairs[-1][1]
            U_alg[6 * b:6 * b + 6, -6:] = 0.0
            kw = dict(U_alg=U_alg)
        return lowrank(self.Bm, self.U, self.B, **kw)

    def certify(self, q=0):
        """band_cond_ref.System.certify on A: (eta of a solve refined with exact residuals, distance of X_ref from it)."""
        x, parts = bc.refined_solve(self.A, self.B[:, q], max_steps=2, exact=True)
        eta = self.eq.eta(self.B[:, q], x, bc.exact_residual(self.A, self.B[:, q], parts))
        return float(eta), float(self.eq.fwd(self.X_ref[:, q], x))

    @functools.cached_property
    def capacitance(self):
        """(Z, C) in f64."""
        return cr.capacitance(self.Bm, self.U)

    @property
    def max_diag_c(self):
        return float(np.diag(self.capacitance[1]).max())


def _weighted(fac, U0, Bm, gamma):
    s = np.sqrt(gamma * np.abs(Bm).max() / float(np.abs(low_rank_term(U0)).max()))
    return scaled(fac, float(s))


def system_name(n, band, tau, where, decades, layout, gamma, stride=1, relative=True):
    return (f"({n},{band}) tau={tau:g} {where}" + (f" units({decades})" if decades else "") + f" {layout} gamma={gamma:g}"
            + (f" stride {stride}" if stride > 1 else "") + ("" if relative else " independent J1"))


@functools.lru_cache(maxsize=48)
def system(n, band, tau, where, decades, layout, gamma, stride=1, relative=True):
    base = bc.system(n, band, tau, where, decades)
    assert n % stride == 0
    rng = np.random.default_rng([2, n, band, LAYOUTS.index(layout), stride])
    fac = random_factors(rng, layout_pairs(layout, n // stride, band // stride + 1), relative)
    fac = _weighted(fac, cr.u_matrix(fac, n, stride), base.A, gamma)
    name = system_name(n, band, tau, where, decades, layout, gamma, stride, relative)
    return ClosureSystem(name, base.A, band, fac, stride, base.B)


COND_BUDGET = {"all": 1e14, "first": 1e12}


def admissible(tau, where, decades, gamma):
    """Whether A = B + U U^T is still a system of f64: the closures weigh gamma against a band system whose weakest
    direction weighs tau (and 10^-2 decades of that under `units`), so cond(A) grows like gamma 10^(2 decades) / tau; the
    prior on pose 0 alone leaves the chain's far end another two decades softer.  Beyond the budget LAPACK does not factor
    A (or refined_solve no longer converges), and neither the widened band nor the low-rank path has a reference."""
    return gamma * 10.0 ** (2 * decades) / tau <= COND_BUDGET[where]


def family(key):
    """(name, accurate, loss ratio, fwd_wood, fwd_direct) of a key of keys(), without holding on to its system."""
    n, band, tau, where, d, layout, gamma, stride = key
    name = system_name(*key)
    if name not in _FAMILY:
        system(*key)
    return (name, *_FAMILY[name])


def keys(shapes=SHAPES, strides=True):
    """The non-bridge keys (module docstring)."""
    out = []
    for n, band in shapes:
        c = 0
        for _, _, tau, where, d in bc.accuracy_keys([(n, band)]):
            for gamma in GAMMAS:
                if admissible(tau, where, d, gamma):
                    out.append((n, band, tau, where, d, LAYOUTS[c % len(LAYOUTS)], gamma, 1))
                    c += 1
    if strides:
        for stride, (n, band) in STRIDE_KEYS.items():
            if (n, band) in shapes:
                for ib, (_, _, tau, where, d) in enumerate(bc.accuracy_keys([(n, band)])):
                    ok = [g for g in GAMMAS if admissible(tau, where, d, g)]
                    out.append((n, band, tau, where, d, LAYOUTS[ib % 2], ok[ib % len(ok)], stride))
    return out


# ---------------------------------------------------------------------------------------------- the bridge family
def bridged(A, n, band, beta):
    """A chain matrix whose factors between nodes < n / 2 and nodes >= n / 2 are weighted by beta.  A pair (i, k) carries
    one factor J^T J = M, stored as -M in the off-diagonal block and added to both diagonal blocks: all four are
    reweighted, so beta = 0 is the chain with those factors left out."""
    out = A.astype(LD)
    cut = n // 2
    for i in range(cut, n):
        for k in range(max(0, i - band), cut):
            si, sk = slice(6 * i, 6 * i + 6), slice(6 * k, 6 * k + 6)
            M = -A[si, sk].astype(LD)
            out[si, si] -= (1 - LD(beta)) * M
            out[sk, sk] -= (1 - LD(beta)) * M
            out[si, sk] = -LD(beta) * M
            out[sk, si] = -LD(beta) * M.T
    return np.asarray(out, dtype=np.float64)


def bridge_pairs(n, band, k):
    """k closures across the cut, more than `band` apart."""
    cut = n // 2
    lo = min(cut - 1, n - 1 - band - 1)
    return [(lo - 2 * f, min(n - 1, lo - 2 * f + band + 1 + 3 * f)) if f % 2 == 0 else
            (min(n - 1, lo - 2 * f + band + 1 + 3 * f), lo - 2 * f) for f in range(k)]


@functools.lru_cache(maxsize=None)
def bridge(n, band, beta, lam, k):
    base = bc.system(n, band, 1e-2, "first")
    Bm = bridged(base.A, n, band, beta) + lam * np.eye(6 * n)
    pairs = bridge_pairs(n, band, k)
    assert all(min(p) < n // 2 <= max(p) for p in pairs)
    rng = np.random.default_rng([3, n, band, k])
    fac = random_factors(rng, pairs)
    fac = _weighted(fac, cr.u_matrix(fac, n), base.A, 1.0)
    return ClosureSystem(f"bridge ({n},{band}) beta={beta:g} lambda={lam:g} k={k}", Bm, band, fac, 1, base.B)


def bridge_keys(shapes=BRIDGE_SHAPES):
    return [(n, band, beta, lam, k) for n, band in shapes for k in BRIDGE_CLOSURES for beta in BETAS for lam in LAMBDAS]


def bridge_line(s):
    """One line of the sweep: fwd_wood, fwd_direct, cond(B + lambda I), cond(A), max diag(C), the family."""
    return (f"{s.name}\t{s.fwd_wood.max():.2e}\t{s.fwd_direct.max():.2e}\t{np.linalg.cond(s.Bm):.2e}\t{np.linalg.cond(s.A):.2e}"
            f"\t{s.max_diag_c:.3e}\t{'accuracy' if s.accurate else 'loss'}")
