"""The band solver's numerics (csrc/band_solve.hip, csrc/marginals.hip) on ill-conditioned, badly scaled, indefinite,
singular and NaN-carrying block bands, against LAPACK and a refined reference on the same system (tests/band_cond_ref.py;
the harness itself is certified on the CPU by tests/test_band_cond_ref.py).  Every bound is a ratio over a value the CPU
computed for that system; the measured values are in profiles/band_conditioning.md.

A line "BCOND <tab> ..." is printed per (system, entry, mode) before its assertion (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import band_cond_ref as bc
import marginals_ref as mr

pytestmark = pytest.mark.gpu

# (cb_max_wg, band_mode): None = automatic; 0 the fused launch per panel; 1 a TRSM + SYRK launch pair; 2 a pair per half
# on two streams; 3 the persistent window kernel, which only the two-sided entries select; cb_max_wg = 3 forces several
# row groups of the back-substitution onto one workgroup
ONE_SIDED_MODES = [(None, None), (None, 0), (None, 1), (None, 2), (3, None)]
SPLIT_MODES = [(None, None), (None, 0), (None, 1), (None, 2), (None, 3), (3, None)]
ENTRY_MODES = [("one", w, m) for w, m in ONE_SIDED_MODES] + [("split", w, m) for w, m in SPLIT_MODES]


def _ids(params):
    return ["-".join(str(v) for v in p) for p in params]


def gpu_solve(d_S, nP, B, rhs, split):
    """Solve A X = rhs ([N, k] on the host, k = 1: the single-right-hand-side entry, which solves S dp = -gs) with the
    factorisation overwriting the device band d_S.  Returns (X [N, k], status)."""
    from visual_underwater_slam_amd import _lib
    lib = _lib.load()
    k = rhs.shape[1]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr()
    work = None
    if split:
        work = torch.empty(max(int(lib.vus_ba_band_solve_work_doubles(nP, B, k)), 1), dtype=torch.float64, device="cuda")
    if k == 1:
        d_g = torch.from_numpy(np.ascontiguousarray(-rhs[:, 0])).cuda()
        d_x = torch.empty(6 * nP, dtype=torch.float64, device="cuda")
        if split:
            _lib.call("vus_ba_band_solve_split", d_S.data_ptr(), nP, B, d_g.data_ptr(), d_x.data_ptr(), st.data_ptr(),
                      work.data_ptr(), stream)
        else:
            _lib.call("vus_ba_band_solve", d_S.data_ptr(), nP, B, d_g.data_ptr(), d_x.data_ptr(), st.data_ptr(), stream)
        return d_x.cpu().numpy()[:, None], int(st.item())
    d_r = torch.from_numpy(np.ascontiguousarray(rhs.T)).cuda()
    if split:
        _lib.call("vus_ba_band_solve_multi_split", d_S.data_ptr(), nP, B, d_r.data_ptr(), k, st.data_ptr(), work.data_ptr(),
                  stream)
    else:
        _lib.call("vus_ba_band_solve_multi", d_S.data_ptr(), nP, B, d_r.data_ptr(), k, st.data_ptr(), stream)
    return d_r.cpu().numpy().T, int(st.item())


def dev(Sb):
    return torch.from_numpy(np.ascontiguousarray(Sb)).cuda()


def split_m(n, band):
    """Poses either half of the two-sided solve eliminates (0: the entry falls back to the one-sided solve): whole panels
    of 8 that leave at least `band` poses in the middle (band_solve.hip, file header).  Checked against the library's own
    answer to "does this size split"."""
    from visual_underwater_slam_amd import _lib
    m = ((n - band) // 2 // 8) * 8 if band > 0 else 0
    m = m if m >= 8 else 0
    assert (int(_lib.load().vus_ba_band_solve_work_doubles(n, band, 1)) > 0) == (m > 0), (n, band)
    return m


# ---------------------------------------------------------------------------------------------- a. accuracy
@pytest.mark.parametrize("entry,max_wg,mode", ENTRY_MODES, ids=_ids(ENTRY_MODES))
def test_accuracy_on_chains_and_badly_scaled_chains(gpu, band_tuning, entry, max_wg, mode):
    """chain and chain + units(3), both prior placements, tau = 1e-2, 1e-5, 1e-8, six shapes; 1 and 7 right-hand sides:
    status 0, finite, eta <= 8 max(eta_LAPACK, 2^-52) and fwd <= 16 max(fwd_LAPACK, 1e-15) on the equilibrated system."""
    band_tuning(band_mode=mode, cb_max_wg=max_wg)
    for key in bc.accuracy_keys():
        s = bc.system(*key)
        for k in (1, bc.N_RHS):
            X, status = gpu_solve(dev(s.Sb), s.n, s.band, s.B[:, :k], entry == "split")
            what = (entry, max_wg, mode, k)
            assert status == 0, (s.label(), what, status)
            finite = np.isfinite(X).all()
            eta = float(s.eq.eta(s.B[:, :k], X).max()) if finite else np.nan
            fwd = float(s.eq.fwd(X, s.X_ref[:, :k]).max()) if finite else np.nan
            print(f"BCOND\tsolve\t{s.label()}\t{entry}\t{max_wg}\t{mode}\t{k}\t{s.cond:.1e}\t{s.eta_lapack.max():.2e}\t{eta:.2e}"
                  f"\t{s.fwd_lapack.max():.2e}\t{fwd:.2e}")
            bc.check_accuracy(s, X, what)


# ---------------------------------------------------------------------------------------------- b. exponent range
@pytest.mark.parametrize("entry,max_wg,mode", ENTRY_MODES, ids=_ids(ENTRY_MODES))
def test_scaling_by_powers_of_four_scales_the_solution_exactly(gpu, band_tuning, entry, max_wg, mode):
    """A 4^k, b 2^k for k = +-250 on every member of chain and chain + units(3) (pivots down to 1e-14 of the diagonal):
    every square root, product and reciprocal of the factorisation scales exactly, so x_scaled 2^k equals the unscaled
    solve of the same mode up to the order of the sweep's atomic additions (1e-12: the project's figure for that, with a
    decade of headroom)."""
    band_tuning(band_mode=mode, cb_max_wg=max_wg)
    for key in bc.accuracy_keys():
        s = bc.system(*key)
        worst = 0.0
        for k in (1, bc.N_RHS):
            X0, st0 = gpu_solve(dev(s.Sb), s.n, s.band, s.B[:, :k], entry == "split")
            assert st0 == 0
            for e in (250, -250):
                Ak, bk = bc.pow4(s.Sb, s.B[:, :k], e)
                X, status = gpu_solve(dev(Ak), s.n, s.band, bk, entry == "split")
                assert status == 0, (s.label(), entry, mode, k, e, status)
                err = bc.relerr(np.ldexp(X, e), X0)
                worst = max(worst, err)
                print(f"BCOND\tpow4\t{s.label()}\t{entry}\t{max_wg}\t{mode}\t{k}\t{e}\t{err:.2e}")
        assert worst <= 1e-12, (s.label(), entry, mode, worst)


# ---------------------------------------------------------------------------------------------- c, d. indefinite systems
@pytest.fixture(scope="module")
def indef():
    """chain(tau = 1e-2 on every pose) of (64,20) and (131,37) with the squared diagonal of the reference factor."""
    out = {}
    for n, band in ((64, 20), (131, 37)):
        s = bc.system(n, band, 1e-2, "all")
        out[n, band] = (s, np.diag(np.linalg.cholesky(s.A)) ** 2, dev(s.Sb))
    return out


def indefinite_status(case, c, k, split):
    """Status of the solve of indefinite(A, c): a copy of the pristine band is patched on the device."""
    s, Lcc2, d_S0 = case
    d_S = d_S0.clone()
    d_S[c // 6, 0, 7 * (c % 6)] = float(s.A[c, c] - 2.0 * Lcc2[c])
    _, status = gpu_solve(d_S, s.n, s.band, s.B[:, :k], split)
    return status


@pytest.mark.parametrize("max_wg,mode", ONE_SIDED_MODES[:4], ids=_ids(ONE_SIDED_MODES[:4]))
def test_one_sided_solve_reports_the_first_negative_pivot(gpu, band_tuning, indef, max_wg, mode):
    """Pivot c = -L_cc^2, pivots before it untouched: status == c + 1 for every column of panel 0, every column of panel 1
    (pivots that exist only after a trailing update), the last column of the last, partial panel of (131,37) and one
    column in each of its thirds."""
    band_tuning(band_mode=mode, cb_max_wg=max_wg)
    for (n, band), cols in (((64, 20), range(96)), ((131, 37), (131, 393, 655, 785))):
        for c in cols:
            for k in (1, bc.N_RHS):
                bc.check_status(indefinite_status(indef[n, band], c, k, False), c, True, (n, band, mode, k))


@pytest.mark.parametrize("max_wg,mode", SPLIT_MODES[:5], ids=_ids(SPLIT_MODES[:5]))
def test_two_sided_solve_reports_a_negative_pivot_in_either_half_and_the_middle(gpu, band_tuning, indef, max_wg, mode):
    """The columns of the one-sided test in each of the three parts of the two-sided solve -- the top-down half, the middle
    system, the bottom-up half: every column of the part's first two panels, the part's last column and the thirds of
    the whole system, on (131,37); on (64,20), whose halves are two panels each, every scalar column.  status > 0
    everywhere; == c + 1 where c lies in the top-down half, whose elimination order is the one-sided one."""
    band_tuning(band_mode=mode, cb_max_wg=max_wg)
    for (n, band) in ((64, 20), (131, 37)):
        m = split_m(n, band)
        assert m > 0
        if n == 64:
            cols = range(6 * n)
        else:
            parts = ((0, 6 * m), (6 * m, 6 * (n - m)), (6 * (n - m), 6 * n))
            cols = sorted({lo + o for lo, hi in parts for o in (*range(96), hi - lo - 1)} | {131, 393, 655, 785})
        for c in cols:
            for k in (1, bc.N_RHS):
                bc.check_status(indefinite_status(indef[n, band], c, k, True), c, c < 6 * m, (n, band, mode, k))


# ---------------------------------------------------------------------------------------------- e. zero and NaN
@pytest.mark.parametrize("entry,max_wg,mode", ENTRY_MODES, ids=_ids(ENTRY_MODES))
def test_zero_pivot_and_nan_are_reported(gpu, band_tuning, entry, max_wg, mode):
    """A pose without factors (its diagonal block and couplings exactly zero): pivot 6 p is 0, status == 6 p + 1.  One NaN
    at the sub-diagonal entry (r, c) inside the band: the first pivot it reaches is r, status == r + 1.  The two-sided
    entries promise some column + 1 > 0, and the one-sided order where the pivot lies in their top-down half."""
    band_tuning(band_mode=mode, cb_max_wg=max_wg)
    split = entry == "split"
    for n, band in bc.SHAPES:
        m = split_m(n, band) if split else 0
        one_sided = not split or m == 0                          # too short to split: the entry falls back
        B = bc.system(n, band, 1e-2, "all").B
        cases = [(6 * p, bc.chain(n, band, 1e-2, "all", isolated=p)) for p in (0, n // 2, n - 1)]
        A = bc.system(n, band, 1e-2, "all").A
        cases += [(r, bc.with_nan(A, r, c)) for r, c in bc.nan_positions(n, band)]
        for col, Ab in cases:
            d_S0 = dev(bc.dense_to_band(Ab, band))
            for k in (1, bc.N_RHS):
                _, status = gpu_solve(d_S0.clone(), n, band, B[:, :k], split)
                bc.check_status(status, col, one_sided or col < 6 * m, (n, band, entry, mode, k))


# ---------------------------------------------------------------------------------------------- f. selected inversion
SELINV_KEYS = bc.accuracy_keys([(23, 7), (64, 20)])


def gpu_selinv(Sb, band):
    """Factor Sb with the one-sided multi solve, then vus_ba_band_selinv: the band of the inverse."""
    from visual_underwater_slam_amd import _lib
    n = Sb.shape[0]
    d_S = dev(Sb)
    rhs = torch.zeros((1, 6 * n), dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.call("vus_ba_band_solve_multi", d_S.data_ptr(), n, band, rhs.data_ptr(), 1, st.data_ptr(), _lib.current_stream_ptr())
    assert int(st.item()) == 0
    nw = int(_lib.load().vus_ba_band_selinv_work_doubles(n, band))
    work = torch.empty(nw, dtype=torch.float64, device="cuda")
    Sg = torch.empty_like(d_S)
    _lib.call("vus_ba_band_selinv", d_S.data_ptr(), n, band, Sg.data_ptr(), work.data_ptr(), nw, _lib.current_stream_ptr())
    return Sg.cpu().numpy()


@pytest.fixture(scope="module")
def selinv_refs():
    """Per system: the refined inverse and the error of marginals_ref.selinv_band (f64 numpy, the same recursion)."""
    out = {}
    for key in SELINV_KEYS:
        s = bc.system(*key)
        Sig = bc.inverse_ref(s.A)
        out[key] = (Sig, bc.selinv_error(mr.selinv_band(s.A, s.band), Sig, s.band))
    return out


@pytest.mark.parametrize("mode", [None, 0, 3])
def test_selected_inversion_on_chains_and_badly_scaled_chains(gpu, band_tuning, selinv_refs, mode):
    """vus_ba_band_selinv behind the one-sided factorisation: entrywise |Sigma_ij - ref_ij| / sqrt(ref_ii ref_jj) over the
    band is at most 16 times that of the f64 numpy statement of the same recursion (floor 1e-15)."""
    band_tuning(band_mode=mode)
    for key in SELINV_KEYS:
        s = bc.system(*key)
        Sig, e_np = selinv_refs[key]
        Sg = gpu_selinv(s.Sb, s.band)
        finite = np.isfinite(Sg).all()
        err = bc.selinv_error(Sg, Sig, s.band) if finite else np.nan
        print(f"BCOND\tselinv\t{s.label()}\t{mode}\t{s.cond:.1e}\t{e_np:.2e}\t{err:.2e}")
        assert finite, (s.label(), mode)
        assert err <= 16 * max(e_np, 1e-15), (s.label(), mode, err, e_np)
