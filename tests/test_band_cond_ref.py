"""The harness of tests/test_band_cond_gpu.py certified on the CPU: the families are what they claim to be, LAPACK is a
sound yardstick on them, the refined reference is a reference, and every shared assertion trips on a real defect."""
import numpy as np
import pytest

import band_cond_ref as bc


def test_chain_has_the_gauge_null_space_and_the_band():
    """Without its prior the chain matrix annihilates the six rigid motions of the whole chain; nothing lies outside the
    band; `isolated` zeroes one pose's block row and column and nothing else."""
    n, band = 23, 7
    A0 = bc.chain(n, band, 1e-2, "first") - np.kron(np.diag([1.0] + [0.0] * (n - 1)), 1e-2 * np.eye(6))
    G = np.tile(np.eye(6), (n, 1))
    assert np.abs(A0 @ G).max() <= 64 * np.finfo(float).eps * np.abs(A0).max()
    assert np.array_equal(bc.band_to_dense(bc.dense_to_band(A0, band)), A0)
    Az = bc.chain(n, band, 1e-2, "all", isolated=11)
    assert not Az[66:72].any() and not Az[:, 66:72].any()
    assert np.linalg.eigvalsh(np.delete(np.delete(Az, np.s_[66:72], 0), np.s_[66:72], 1)).min() > 0


@pytest.mark.parametrize("shape", bc.SHAPES)
def test_lapack_is_backward_stable_and_the_refined_solve_is_a_reference(shape):
    """Every case: LAPACK factorises it with eta <= 4 * 2^-52 and cond(A) <= 1e13 before `units`.  The reference: for
    right-hand side 0 of every system (the only column certified this way: the exact sums are slow), a refined solve whose
    residuals are summed exactly has eta <= 1e-3 of LAPACK's (np.longdouble cannot show that: its resolution,
    2^-64, is only 2^-11 below f64's), and the np.longdouble-refined X_ref the GPU tests compare with lies within 1 % of the
    forward-error bound it is used to check, so its own error cannot decide that check."""
    for key in bc.accuracy_keys([shape]):
        s = bc.system(*key)
        assert bc.lapack_status(s.A) == 0, s.label()
        assert s.eta_lapack.max() <= 4 * bc.EPS, (s.label(), s.eta_lapack.max())
        eta_ref, dist = s.certify(0)
        assert eta_ref <= 1e-3 * s.eta_lapack[0], (s.label(), eta_ref, s.eta_lapack[0])
        assert dist <= 0.01 * bc.fwd_bound(s.fwd_lapack), (s.label(), dist, bc.fwd_bound(s.fwd_lapack))
        if key[4] == 0:
            assert s.cond <= 1e13, (s.label(), s.cond)
        # LAPACK itself passes the assertion the GPU solver is held to
        bc.check_accuracy(s, s.X_lapack, "LAPACK")


def test_refined_solve_agrees_with_a_50_digit_cholesky():
    """(23,7), tau = 1e-8 on pose 0 only: the refined solve against an mpmath Cholesky solve at 50 digits, to 1e-3 of
    LAPACK's forward error."""
    import mpmath
    s = bc.system(23, 7, 1e-8, "first")
    with mpmath.workdps(50):
        x = mpmath.cholesky_solve(mpmath.matrix(s.A.tolist()), mpmath.matrix(s.B[:, 0].tolist()))
        x_mp = np.array([bc.LD(mpmath.nstr(v, 25)) for v in x])
    fwd_lapack = s.eq.fwd(s.X_lapack[:, 0], x_mp)
    fwd_ref = s.eq.fwd(s.X_ref[:, 0], x_mp)
    assert fwd_ref <= 1e-3 * fwd_lapack, (fwd_ref, fwd_lapack)


@pytest.mark.parametrize("n,band,cols", [(64, 20, range(96)), (131, 37, (131, 393, 655, 785))])
def test_lapack_reports_the_leading_minor_of_an_indefinite_case(n, band, cols):
    A = bc.chain(n, band, 1e-2, "all")
    L = np.linalg.cholesky(A)
    for c in cols:
        Ai = bc.indefinite(A, c, L)
        assert bc.lapack_status(Ai) == c + 1
        if c % 16 == 0:      # the plain statement of "carry on and note the first one" agrees (a sample: it is O(N^3) Python)
            assert bc.first_bad_pivot(Ai) == c + 1
        bc.check_status(bc.lapack_status(Ai), c, exact=True)


def test_zero_and_nan_cases_have_the_pivots_the_gpu_test_expects():
    n, band = 23, 7
    for p in (0, n // 2, n - 1):
        assert bc.first_bad_pivot(bc.chain(n, band, 1e-2, "all", isolated=p)) == 6 * p + 1
    A = bc.chain(n, band, 1e-2, "all")
    for r, c in bc.nan_positions(n, band):
        assert r > c and (r // 6 - c // 6) <= band
        assert bc.first_bad_pivot(bc.with_nan(A, r, c)) == r + 1


def test_pow4_scales_a_solve_exactly():
    s = bc.system(23, 7, 1e-2, "all", 3)
    for k in (250, -250):
        Ak, bk = bc.pow4(s.A, s.B, k)
        assert np.isfinite(Ak).all() and (Ak[s.A != 0] != 0).all()
        assert bc.relerr(np.ldexp(bc.lapack_solve(Ak, bk), k), s.X_lapack) <= 1e-12


@pytest.mark.parametrize("key", [(23, 7, 1e-2, "all", 0), (23, 7, 1e-5, "first", 0), (64, 20, 1e-5, "first", 3),
                                 (131, 37, 1e-2, "all", 3)])
def test_accuracy_assertion_trips_on_24_bit_pivot_reciprocals(key):
    """f64 Cholesky with every pivot reciprocal rounded to 24 bits -- the solver without the correction step behind
    v_rsq_f64 -- fails check_accuracy; the same code with 53 bits passes it."""
    s = bc.system(*key)
    bc.check_accuracy(s, bc.degraded_solve(s.A, s.B, bits=53), "53 bits")
    X = bc.degraded_solve(s.A, s.B, bits=24)
    assert np.isfinite(X).all() and s.eq.eta(s.B, X).max() > 1e3 * bc.eta_bound(s.eta_lapack)
    with pytest.raises(AssertionError):
        bc.check_accuracy(s, X, "24 bits")
    with pytest.raises(AssertionError):
        bc.check_accuracy(s, np.where(np.arange(6 * s.n)[:, None] == 5, np.nan, s.X_lapack), "NaN")


def test_status_assertion_trips_on_an_off_by_one_status():
    for c in (0, 47, 48, 785):
        bc.check_status(c + 1, c, exact=True)
        bc.check_status(c + 7, c, exact=False)
        for wrong in (c, c + 2, 0, -1):
            with pytest.raises(AssertionError):
                bc.check_status(wrong, c, exact=True)
        for wrong in (0, -1, -3):
            with pytest.raises(AssertionError):
                bc.check_status(wrong, c, exact=False)


def test_selected_inversion_reference_and_its_assertion():
    """The refined inverse is a better inverse than numpy's, marginals_ref.selinv_band lies within its own round-off of it,
    and the entrywise measure sees a band whose diagonal panels came from 24-bit reciprocals."""
    import marginals_ref as mr
    s = bc.system(23, 7, 1e-5, "first", 3)
    Sig = bc.inverse_ref(s.A)
    Al = s.A.astype(bc.LD)
    I = np.eye(6 * s.n)
    assert np.abs(Al @ Sig - I).max() <= 1e-3 * np.abs(Al @ np.linalg.inv(s.A).astype(bc.LD) - I).max()
    e_np = bc.selinv_error(mr.selinv_band(s.A, s.band), Sig, s.band)
    assert e_np <= 1e-3
    bad = bc.degraded_solve(s.A, I, bits=24)
    assert bc.selinv_error(mr.dense_to_band(bad, s.band), Sig, s.band) > 16 * max(e_np, 1e-15)
