"""The harness of tests/test_fixed_lag_cond_gpu.py certified on the CPU: the families are what they claim to be, every listed
system is usable, the refined Schur complement is a reference, the numpy statement meets its own bounds, and every shared
assertion trips on a deliberately wrong marginalisation."""
import numpy as np
import pytest

import band_cond_ref as bc
import fixed_lag_cond_ref as fc
import fixed_lag_nav_ref as fn


def test_free_chain_is_gauge_free_and_its_head_is_grounded_by_the_kept_part():
    n, band, k = 23, 7, 17
    A = fc.free_chain(n, band)
    Z = np.tile(np.eye(6), (n, 1))
    assert np.abs(A @ Z).max() <= 64 * bc.EPS * np.abs(A).max()
    assert np.array_equal(bc.band_to_dense(bc.dense_to_band(A, band)), A)
    ev = np.linalg.eigvalsh(A)
    assert (np.abs(ev[:6]) <= 1e-12 * ev[-1]).all() and ev[6] > 1e-6 * ev[-1]          # exactly six free directions
    assert np.linalg.eigvalsh(A[:6 * k, :6 * k])[0] > 0
    # the units scaling moves the null space to D^-1 Z, which has the columns of Z: H Z = 0 still
    assert np.abs(bc.units(A, 3) @ Z @ np.diag([1, 1, 1, 1e3, 1e3, 1e3])).max() <= 64 * bc.EPS * np.abs(A).max()


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_every_accuracy_system_is_usable(shape):
    """Every system of the accuracy and exponent tests: S_MM factors on the CPU; the numpy statement meets the bounds the GPU
    is held to with the factor 16 replaced by 1; the kernel's arithmetic in numpy (another order of the same sums) passes
    the checks the GPU is held to."""
    for key in fc.accuracy_keys([shape]):
        s = fc.system(*key)
        assert bc.lapack_status(s.A[:s.K, :s.K]) == 0 and fc.cpu_status(s.A, s.n_drop) == 0, s.label()
        assert np.isfinite(s.cond) and s.cond < 1e12, (s.label(), s.cond)
        H, g, quad, status = s.numpy
        assert status == 0
        fc.check_marginal((H, g, quad), s, factor=1.0, what="numpy")
        fc.check_psd(H, s, factor=1.0, what="numpy")
        if s.free:
            fc.check_null(H, s, factor=1.0, what="numpy")
            assert fc.lam_min(s.A[s.K:, s.K:], s.diag_RR) > 0           # S_RR itself is definite: the zero modes are H's own
        if shape[0] <= 64 or key[3:] == (None, None, 3):
            Hp, gp, qp, st = fc.panel_marginal(s.A, s.b, s.n_drop)
            assert st == 0
            fc.check_marginal((Hp, gp, qp), s, what="panel arithmetic")
            fc.check_psd(Hp, s, what="panel arithmetic")
    for key in fc.accuracy_keys([shape]) if shape in fc.POW4_SHAPES else ():
        s = fc.system(*key)
        for e in (250, -250):
            Ak, bk = bc.pow4(s.A, s.b, e)
            assert np.isfinite(Ak).all() and np.array_equal(np.ldexp(Ak, -2 * e), s.A) and np.array_equal(np.ldexp(bk, -e), s.b)


def test_the_refined_marginal_agrees_with_a_50_digit_schur_complement():
    """(9,2,6), the anchor tau = 1e-8 inside the dropped head, units(3): marginal_ref against mpmath at 50 digits lies within
    1e-3 of the bound it is used to check, so its own error cannot decide that check."""
    import mpmath
    s = fc.system(9, 2, 6, 1e-8, "first", 3)
    K = s.K
    with mpmath.workdps(50):
        A, b = mpmath.matrix(s.A.tolist()), mpmath.matrix(s.b.tolist())
        rhs = mpmath.matrix(K, len(s.b) - K + 1)
        for i in range(K):
            for j in range(len(s.b) - K):
                rhs[i, j] = A[i, K + j]
            rhs[i, len(s.b) - K] = b[i]
        X = mpmath.matrix(K, rhs.cols)
        for j in range(rhs.cols):
            X[:, j] = mpmath.lu_solve(A[:K, :K], rhs[:, j])
        H = A[K:, K:] - A[K:, :K] * X[:, :len(s.b) - K]
        g = b[K:, 0] - A[K:, :K] * X[:, len(s.b) - K]
        quad = (b[:K, 0].T * X[:, len(s.b) - K])[0]
        to_ld = lambda M: np.array([[bc.LD(mpmath.nstr(M[i, j], 25)) for j in range(M.cols)] for i in range(M.rows)])
        exact = (to_ld(H), to_ld(g)[:, 0], bc.LD(mpmath.nstr(quad, 25)))
    e = [fc.cw_err(got, ex, mag) for got, ex, mag in zip(s.ref[:3], exact, s.ref[3:])]
    for got_e, np_e in zip(e, s.err_numpy):
        assert got_e <= 1e-3 * fc.bound(np_e), (e, s.err_numpy)


def test_the_error_measures_guard_zero_rows():
    """A kept node that no absorbed factor touches has an exactly zero row: legal, measured as 0, and anything but an exact
    zero there is an infinite error."""
    r = fc.recursion(*fc.RECURSIONS[0])
    ref = r.one_shot
    zero = ref.magH == 0
    assert zero.any() and (np.asarray(ref.H)[zero] == 0).all() and (r.diag_RR == 0).any()
    H = np.asarray(ref.H, dtype=np.float64)
    assert fc.cw_err(H, ref.H, ref.magH) <= bc.EPS
    H[np.nonzero(zero)[0][0], np.nonzero(zero)[1][0]] = 1e-300
    assert fc.cw_err(H, ref.H, ref.magH) == float("inf")
    assert np.isfinite(fc.lam_min(np.asarray(ref.H, dtype=np.float64), r.diag_RR))


@pytest.mark.parametrize("key", fc.RECURSIONS + (fc.PADDED_RECURSION + (3, True),))
def test_every_recursion_is_usable(key):
    """The numpy statement never fails its Cholesky over the T steps, stays at errH <= 1e-13 against the one-shot reference
    with an equilibrated lambda_min >= -1e-13, produces priors vus_window_prior_check would accept at every step, and the
    kernel's arithmetic in numpy passes the check the GPU is held to."""
    r = fc.recursion(*key)
    ny = r.numpy
    assert ny["err"][0] <= 1e-13 and ny["lam"] >= -1e-13, (r.label(), ny["err"], ny["lam"])
    assert np.isfinite(r.cond) and r.cond < 1e11

    def each(t, A, b, H, g, status):
        assert status == 0 and fc.cpu_status(A, r.n_drop) == 0, (r.label(), t)
        fc.check_prior(H, g, (r.label(), t))
        if r.padded:
            _, _, dev = fn.compact(H, g)
            assert dev == 0.0, (r.label(), t, dev)
    got = r.run(fc.panel_marginal, each)
    r.check(got, what="panel arithmetic")
    r.check((ny["H"], ny["g"], ny["quad"]), factor=1.0, what="numpy")
    if r.tau == 0:
        assert ny["null"] <= 1e-12


# ---------------------------------------------------------------------------------------------- wrong on purpose
WELL = (23, 7, 17, 1e-2, "all", 0)


def test_rounded_pivot_reciprocals_fail_the_accuracy_check():
    for key in (WELL, (23, 7, 17, None, None, 0), (64, 20, 45, 1e-5, "first", 0)):
        s = fc.system(*key)
        fc.check_marginal(fc.panel_marginal(s.A, s.b, s.n_drop)[:3], s)
        with pytest.raises(AssertionError, match="err"):
            fc.check_marginal(fc.panel_marginal(s.A, s.b, s.n_drop, inv_bits=24)[:3], s)


def test_a_skipped_partial_panel_fails_the_accuracy_check():
    """n_drop = 17 and 45: two and five whole panels and a partial one.  With n_drop = 16 (whole panels only) the same
    variant is right, which shows what it skips."""
    for key in (WELL, (64, 20, 45, 1e-2, "all", 3)):
        s = fc.system(*key)
        with pytest.raises(AssertionError, match="errH"):
            fc.check_marginal(fc.panel_marginal(s.A, s.b, s.n_drop, skip_partial=True)[:3], s)
    s = fc.system(23, 7, 16, 1e-2, "all", 0)
    fc.check_marginal(fc.panel_marginal(s.A, s.b, s.n_drop, skip_partial=True)[:3], s)


def test_a_gradient_row_left_out_of_the_update_fails_on_g_alone():
    s = fc.system(*WELL)
    H, g, quad, _ = fc.panel_marginal(s.A, s.b, s.n_drop, skip_gradient=True)
    eH, eg, eq = fc.errors((H, g, quad), s.ref)
    assert eH <= fc.bound(s.err_numpy[0]) and eg > fc.bound(s.err_numpy[1])
    with pytest.raises(AssertionError, match="errg"):
        fc.check_marginal((H, g, quad), s)


def test_the_status_check_rejects_an_off_by_one_and_a_whole_matrix_status():
    """chain(64, 20, 1e-2, all), n_drop = 45: LAPACK's leading-minor order of S_MM is the expected status for every listed
    column, the carry-on Cholesky of band_cond_ref agrees on a sample; a status one short, and the first bad pivot of the whole
    matrix in place of S_MM's, are both refused."""
    s = fc.system(64, 20, 45, 1e-2, "all", 0)
    N, K = 6 * s.n, s.K
    L = np.linalg.cholesky(s.A)
    cols = fc.status_columns(N, K)
    assert set(range(96)) <= set(cols) and {K - 1, K, N - 1, 96, 143, 240, 269} <= set(cols)
    for c in cols:
        Ai = bc.indefinite(s.A, c, L)
        fc.check_status(bc.lapack_status(Ai[:K, :K]), c, K)
    big = fc.system(131, 37, 93, 1e-2, "all", 0)                      # the other status system: the same by LAPACK
    Lb = np.linalg.cholesky(big.A)
    for c in fc.status_columns(6 * big.n, big.K):
        fc.check_status(bc.lapack_status(bc.indefinite(big.A, c, Lb)[:big.K, :big.K]), c, big.K)
    for c in (0, 5, 47, 48, 95, 96, K - 1, K, N - 1):
        Ai = bc.indefinite(s.A, c, L)
        good = fc.cpu_status(Ai, s.n_drop)
        fc.check_status(good, c, K)
        assert fc.panel_marginal(Ai, s.b, s.n_drop)[3] == good
        if c < K:
            with pytest.raises(AssertionError, match="status"):
                fc.check_status(good - 1, c, K)
        else:
            with pytest.raises(AssertionError, match="status"):
                fc.check_status(bc.first_bad_pivot(Ai), c, K)
            H = fc.panel_marginal(Ai, s.b, s.n_drop)[0]            # the status is 0 and H is indefinite
            assert fc.lam_min(H, s.diag_RR) < fc.psd_bound(s.lam_numpy, N - K)
    # an isolated dropped pose and a NaN: the same convention
    for p in (0, s.n_drop // 2, s.n_drop - 1):
        assert fc.cpu_status(bc.chain(64, 20, 1e-2, "all", isolated=p), s.n_drop) == 6 * p + 1
    head, tail = fc.nan_entries(s.n, s.band, s.n_drop)
    for r, c in head:
        assert c < r < K and fc.cpu_status(bc.with_nan(s.A, r, c), s.n_drop) == r + 1
    for r, c in tail:
        assert r >= K and r > c and (r // 6 - c // 6) <= s.band
        An = bc.with_nan(s.A, r, c)
        H, _, _, st = fc.panel_marginal(An, s.b, s.n_drop)
        assert fc.cpu_status(An, s.n_drop) == 0 and st == 0 and np.isnan(H).any()


def test_a_recursion_that_mirrors_the_stale_triangle_fails_the_recursion_check():
    import functools
    r = fc.recursion(*fc.RECURSIONS[0])
    with pytest.raises(AssertionError, match="errH"):
        r.check(r.run(functools.partial(fc.panel_marginal, stale_triangle=True)))
    # ... and a recursion with 24-bit pivot reciprocals drifts out of the bound as well
    with pytest.raises(AssertionError, match="err"):
        r.check(r.run(functools.partial(fc.panel_marginal, inv_bits=24)))


def test_the_prior_family_references():
    """The priors of the family tests have the sizes the kernels' second passes need, are symmetric with a non-negative
    diagonal, and the np.longdouble energy agrees with f64 to round-off of its magnitude sum."""
    for rows in (66, 258, 75, 270):
        for kind in fc.PRIOR_KINDS:
            H, g, c = fc.prior_of(rows, kind)
            assert H.shape == (rows, rows) and np.array_equal(H, H.T)
            fc.check_prior(H, g, (rows, kind))
            u = 0.03 * np.random.default_rng(rows).normal(size=rows)
            grad, e, mg, me = fc.prior_energy_ref(H, g, c, u)
            assert fc.cw_err(g + H @ u, grad, mg) <= 64 * bc.EPS
            assert fc.cw_err(c + g @ u + 0.5 * u @ H @ u, e, me) <= 64 * bc.EPS
    assert 66 > 64 and 258 + 1 > 256 and 270 + 1 > 256
