"""The numerics of fixed-lag marginalisation (csrc/fixed_lag.hip, csrc/fixed_lag_nav.hip) on ill-conditioned, badly scaled and
gauge-free systems, at the sizes where the kernels take their second passes, and through 100+ steps of the recursion in which
every output is the next input -- against the refined np.longdouble reference of tests/fixed_lag_cond_ref.py (certified on the
CPU by tests/test_fixed_lag_cond_ref.py).  Every bound is a ratio (16, floor 1e-15) over what the f64 numpy statement of
fixed_lag_ref.py reaches on the same system; the measured values are in profiles/fixed_lag_conditioning.md.

A line "FLCOND <tab> ..." is printed per (system, check) before its assertion (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import band_cond_ref as bc
import fixed_lag_cond_ref as fc
import fixed_lag_nav_ref as fn
import fixed_lag_ref as fl
import nav_bias_ref as nbr

pytestmark = pytest.mark.gpu

F64 = dict(dtype=torch.float64, device="cuda")
I12 = np.r_[np.eye(3).reshape(-1), np.zeros(3)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def ratio(got, numpy_value):
    return got / max(numpy_value, fc.FLOOR)


def gpu_marginalize(d_S, d_g, n, band, k):
    """vus_ba_band_marginalize on a device band: (H, g, quad, status) on the host.  The outputs are pre-filled with NaN and
    the status word with -7."""
    from visual_underwater_slam_amd import _lib
    w = n - k
    H = torch.full((6 * w, 6 * w), float("nan"), **F64)
    g = torch.full((6 * w,), float("nan"), **F64)
    quad = torch.full((1,), float("nan"), **F64)
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().vus_ba_band_marginalize_work_doubles(n, band, k)), **F64)
    assert work.numel() > 0
    p = _lib.ptr
    _lib.call("vus_ba_band_marginalize", p(d_S), n, band, p(d_g), k, p(H), p(g), p(quad), p(status), p(work), _lib.current_stream_ptr())
    return H.cpu().numpy(), g.cpu().numpy(), float(quad.item()), int(status.item())


def marginalize_dense(A, b, k, band=None):
    """The same from a dense host system over A.shape[0] / 6 nodes (band: that of the matrix; default the full triangle)."""
    n = A.shape[0] // 6
    band = n - 1 if band is None else band
    return gpu_marginalize(dev(bc.dense_to_band(A, band)), dev(b.reshape(n, 6)), n, band, k)


def prior_check(H, g, band=None):
    """WindowPrior + vus_window_prior_check on a host (H, g) over identity poses."""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import WindowPrior
    m = len(g) // 6
    W = WindowPrior(0, np.tile(I12, (m, 1)), H, g, 0.0, m)
    _lib.call("vus_window_prior_check", W.addr(), m - 1 if band is None else band, _lib.current_stream_ptr())
    torch.cuda.synchronize()


def _label(key):
    return fc.label_of(key).replace(" ", "_") if len(key) == 6 else "-".join(str(v) for v in key)


# ---------------------------------------------------------------------------------------------- a. accuracy
@pytest.mark.parametrize("key", fc.accuracy_keys(), ids=_label)
def test_marginalize_on_ill_conditioned_badly_scaled_and_gauge_free_systems(gpu, key):
    """chain(tau = 1e-2, 1e-5, 1e-8 on pose 0 -- inside the dropped head -- or on every pose) and free_chain, plain and under
    units(3), nine shapes: status 0; finite, bit-symmetric, errH, errg, errq <= 16 max(numpy, 1e-15); the equilibrated
    lambda_min >= -16 max(-numpy's, 6 w 2^-52); on free_chain |H Z| / (|H| |Z|) <= 16 max(numpy's, 1e-15); two calls give the
    same bits."""
    s = fc.system(*key)
    d_S, d_g = dev(s.Sb), dev(s.b.reshape(s.n, 6))
    H, g, quad, status = gpu_marginalize(d_S, d_g, s.n, s.band, s.n_drop)
    finite = np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(quad)
    e = fc.errors((H, g, quad), s.ref) if finite else (np.nan,) * 3
    lam = fc.lam_min(H, s.diag_RR) if finite else np.nan
    nul = fc.null_err(H) if finite and s.free else np.nan
    en = s.err_numpy
    print(f"FLCOND\tmarginal\t{s.label()}\t{s.cond:.1e}\t" + "\t".join(f"{a:.2e}\t{b:.2e}\t{ratio(b, a):.2f}" for a, b in zip(en, e))
          + f"\t{s.lam_numpy:.2e}\t{lam:.2e}\t{s.null_numpy if s.free else np.nan:.2e}\t{nul:.2e}\t{status}")
    assert status == 0, (s.label(), status)
    fc.check_marginal((H, g, quad), s)
    fc.check_psd(H, s)
    if s.free:
        fc.check_null(H, s)
    again = gpu_marginalize(d_S, d_g, s.n, s.band, s.n_drop)
    assert np.array_equal(H, again[0]) and np.array_equal(g, again[1]) and quad == again[2] and again[3] == 0


# ---------------------------------------------------------------------------------------------- b. exponent range
@pytest.mark.parametrize("key", fc.accuracy_keys(fc.POW4_SHAPES), ids=_label)
def test_scaling_by_powers_of_four_scales_the_marginal_exactly(gpu, key):
    """A 4^e, b 2^e for e = +-250: H 4^-e, g 2^-e and quad equal the unscaled call's to 1e-12 relative (the band solve's
    figure for the same property).  Every operation of the kernel scales exactly and the summation order is fixed: whether
    the results were bit-identical is printed."""
    s = fc.system(*key)
    H0, g0, q0, st0 = gpu_marginalize(dev(s.Sb), dev(s.b.reshape(s.n, 6)), s.n, s.band, s.n_drop)
    assert st0 == 0
    worst = 0.0
    for e in (250, -250):
        Ak, bk = bc.pow4(s.Sb, s.b, e)
        H, g, q, status = gpu_marginalize(dev(Ak), dev(bk.reshape(s.n, 6)), s.n, s.band, s.n_drop)
        Hs, gs = np.ldexp(H, -2 * e), np.ldexp(g, -e)
        err = max(bc.relerr(Hs, H0), bc.relerr(gs, g0), abs(q - q0) / abs(q0))
        exact = np.array_equal(Hs, H0) and np.array_equal(gs, g0) and q == q0
        print(f"FLCOND\tpow4\t{s.label()}\t{e}\t{err:.2e}\t{'bit-exact' if exact else 'differs'}\t{status}")
        assert status == 0, (s.label(), e, status)
        worst = max(worst, err)
    assert worst <= 1e-12, (s.label(), worst)


# ---------------------------------------------------------------------------------------------- c. status
STATUS_SYSTEMS = ((64, 20, 45), (131, 37, 93))


@pytest.fixture(scope="module")
def indef():
    """chain(tau = 1e-2 on every pose) of (64,20) dropping 45 and (131,37) dropping 93, with the squared diagonal of the
    reference factor of the whole matrix and the band on the device."""
    out = {}
    for shape in STATUS_SYSTEMS:
        s = fc.system(*shape, 1e-2, "all")
        out[shape] = (s, np.diag(np.linalg.cholesky(s.A)) ** 2, dev(s.Sb), dev(s.b.reshape(s.n, 6)))
    return out


@pytest.mark.parametrize("shape", STATUS_SYSTEMS, ids=_label)
def test_status_names_the_first_negative_pivot_of_the_dropped_part_only(gpu, indef, shape):
    """Pivot c = -L_cc^2 (patched on a device copy), pivots before it untouched: status == c + 1 for every column of panels
    0 and 1, the first and last column of every later panel and the last column K - 1 of the partial panel.  c = K and
    c = N - 1 lie in the kept part, which the kernel does not factor: status == 0 and H has a negative equilibrated
    eigenvalue -- the status speaks of S_MM only."""
    s, Lcc2, d_S0, d_g = indef[shape]
    N, K = 6 * s.n, s.K
    cols = fc.status_columns(N, K)
    assert K % fc.PW and len(cols) >= 96 + 2 * (K // fc.PW - 2) + 3
    seen = []
    for c in cols:
        d_S = d_S0.clone()
        d_S[c // 6, 0, 7 * (c % 6)] = float(s.A[c, c] - 2.0 * Lcc2[c])
        H, g, quad, status = gpu_marginalize(d_S, d_g, s.n, s.band, s.n_drop)
        seen.append((c, status))
        if c >= K:
            lam = fc.lam_min(H, s.diag_RR)
            print(f"FLCOND\tstatus-kept\t{s.label()}\t{c}\t{status}\t{lam:.2e}")
            assert np.isfinite(H).all() and lam < fc.psd_bound(s.lam_numpy, N - K), (s.label(), c, lam)
    bad = [(c, st) for c, st in seen if st != fc.expected_status(c, K)]
    print(f"FLCOND\tstatus\t{s.label()}\t{len(cols)} columns\t{len(bad)} wrong")
    for c, status in seen:
        fc.check_status(status, c, K, s.label())


@pytest.mark.parametrize("shape", STATUS_SYSTEMS, ids=_label)
def test_status_names_a_dropped_pose_without_information_and_a_nan(gpu, indef, shape):
    """A dropped pose without factors: status == 6 p + 1.  A NaN at a sub-diagonal entry (r, c): with r < K the first pivot
    it reaches is r, status == r + 1, the carry-on Cholesky of S_MM on the CPU says the same; with r >= K (in S_RR or S_RM)
    status == 0, H carries the NaN and vus_window_prior_check refuses the prior as "not finite"."""
    from visual_underwater_slam_amd import _lib
    s = indef[shape][0]
    n, band, k = shape
    for p in (0, k // 2, k - 1):
        Ai = bc.chain(n, band, 1e-2, "all", isolated=p)
        *_, status = marginalize_dense(Ai, s.b, k, band)
        print(f"FLCOND\tisolated\t{s.label()}\t{p}\t{status}")
        assert status == 6 * p + 1, (s.label(), p, status)
    head, tail = fc.nan_entries(n, band, k)
    for r, c in head:
        An = bc.with_nan(s.A, r, c)
        *_, status = marginalize_dense(An, s.b, k, band)
        print(f"FLCOND\tnan-dropped\t{s.label()}\t{(r, c)}\t{status}")
        assert status == r + 1 == fc.cpu_status(An, k), (s.label(), r, c, status)
    for r, c in tail:
        H, g, quad, status = marginalize_dense(bc.with_nan(s.A, r, c), s.b, k, band)
        print(f"FLCOND\tnan-kept\t{s.label()}\t{(r, c)}\t{status}\t{int(np.isnan(H).sum())} NaN in H")
        assert status == 0 and np.isnan(H).any(), (s.label(), r, c, status)
        with pytest.raises(_lib.VusError, match="not finite"):
            prior_check(H, g)


# ---------------------------------------------------------------------------------------------- d. the recursion
def _report(r, got, what):
    e = fc.errors(got, r.one_shot)
    ny = r.numpy
    lam = fc.lam_min(got[0], r.diag_RR)
    nul = fc.null_err(got[0]) if r.tau == 0 and not r.padded else np.nan
    print(f"FLCOND\t{what}\t{r.label()}\t{r.cond:.1e}\t" + "\t".join(f"{a:.2e}\t{b:.2e}\t{ratio(b, a):.2f}" for a, b in zip(ny["err"], e))
          + f"\t{ny['lam']:.2e}\t{lam:.2e}\t{ny['null']:.2e}\t{nul:.2e}")


@pytest.mark.parametrize("key", fc.RECURSIONS, ids=_label)
def test_a_prior_carried_through_100_marginalisations_stays_on_the_one_shot_marginal(gpu, key):
    """fixed_lag_cond_ref.Recursion with vus_ba_band_marginalize as the step; the band of every step is built on the HOST
    with plain f64 additions (prior + factors, the same sums the numpy recursion sees) and uploaded.  Every step: status 0
    and what vus_window_prior_check enforces (finite, diagonal >= 0, asymmetry <= 1e-12 hmax; in fact bit-symmetric); every
    25th step the check itself.  After T steps errH, errg and the accumulated constant against the ONE-SHOT marginal of all
    absorbed factors are <= 16 max(the numpy recursion's, 1e-15); the PSD bound and, for tau = 0, the null-space bound hold."""
    r = fc.recursion(*key)

    def each(t, A, b, H, g, status):
        assert status == 0, (r.label(), t, status)
        fc.check_prior(H, g, (r.label(), t))
        assert np.array_equal(H, H.T), (r.label(), t)
        if t % 25 == 24:
            prior_check(H, g)
    got = r.run(marginalize_dense, each)
    _report(r, got, "recursion")
    r.check(got)


def test_the_recursion_with_velocity_padding_keeps_exact_identity_rows(gpu):
    """Three nodes (a keyframe X, V, B) dropped per step on a system with the identity padding of velocity nodes; each step's
    result goes through vus_nav_window_prior_compact and comes back from its 15-coordinate form.  The kept padding rows are
    exact identity rows with a zero gradient, the compaction equals fixed_lag_nav_ref.compact bit for bit with dev == 0, and
    the final prior meets the bounds of the recursion test."""
    from visual_underwater_slam_amd import _lib
    r = fc.recursion(*fc.PADDED_RECURSION, 3, True)
    wk = r.band // 3
    rows, pad = fn.rows(0, wk), fn.pad_rows(0, wk)
    eye = np.eye(6 * r.band)
    p = _lib.ptr

    def step(A, b, k):
        H, g, quad, status = marginalize_dense(A, b, k)
        assert status == 0 and np.isfinite(H).all()
        assert np.array_equal(H[pad], eye[pad]) and np.array_equal(H[:, pad], eye[:, pad]) and not g[pad].any()
        H15, g15 = torch.full((15 * wk, 15 * wk), float("nan"), **F64), torch.full((15 * wk,), float("nan"), **F64)
        d_H, d_g = dev(H), dev(g)
        _lib.call("vus_nav_window_prior_compact", p(d_H), p(d_g), wk, p(H15), p(g15), _lib.current_stream_ptr())
        Hc, gc, dv = fn.compact(H, g)
        assert dv == 0.0 and np.array_equal(H15.cpu().numpy(), Hc) and np.array_equal(g15.cpu().numpy(), gc)
        H18, g18 = eye * 0.0, np.zeros(6 * r.band)
        H18[np.ix_(rows, rows)] = H15.cpu().numpy()
        g18[rows] = g15.cpu().numpy()
        H18[pad, pad] = 1.0
        return H18, g18, quad, status
    got = r.run(step, lambda t, A, b, H, g, status: fc.check_prior(H, g, (r.label(), t)))
    _report(r, got, "recursion-padded")
    r.check(got)


# ---------------------------------------------------------------------------------------------- e. the prior families
def _energy_line(what, tag, names, refs, mags, numpy_values, gpu_values):
    """Prints the FLCOND line of one prior and asserts every figure: |gpu - ref| / mag <= 16 max(the numpy statement's, 1e-15)."""
    fig = [(n, fc.cw_err(a, r, m), fc.cw_err(b, r, m)) for n, r, m, a, b in zip(names, refs, mags, numpy_values, gpu_values)]
    print(f"FLCOND\t{what}\t{tag}\t" + "\t".join(f"{n}\t{en:.2e}\t{eg:.2e}\t{ratio(eg, en):.2f}" for n, en, eg in fig))
    for n, en, eg in fig:
        assert eg <= fc.bound(en), (what, tag, n, eg, "bound", fc.bound(en))


def _window_mask(n_nodes, band, node_rows):
    """Entries of Sband [n_nodes, band + 1, 36] inside the blocks spanned by the scalar rows `node_rows` (both indices)."""
    E = np.zeros((6 * n_nodes, 6 * n_nodes))
    E[np.ix_(node_rows, node_rows)] = 1.0
    return nbr.band_blocks(E, n_nodes, band) != 0.0


def _assemble_check(S0, g0, S1, g1, Hbig, grad_big, inside_S, inside_g):
    """S1 = S0 + the blocks of H and g1 = g0 + grad to 1 ulp of the sum; everything outside the window bit-identical."""
    wantS, wantg = S0 + Hbig, g0 + grad_big
    assert (np.abs(S1 - wantS) <= np.spacing(np.abs(wantS)))[inside_S].all()
    assert (np.abs(g1 - wantg) <= np.spacing(np.abs(wantg)))[inside_g].all()
    assert np.array_equal(S1[~inside_S].view(np.int64), S0[~inside_S].view(np.int64))
    assert np.array_equal(g1[~inside_g].view(np.int64), g0[~inside_g].view(np.int64))


@pytest.mark.parametrize("kind", fc.PRIOR_KINDS)
@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("m", [11, 43])
def test_window_prior_at_sizes_with_a_second_pass_and_a_second_energy_workgroup(gpu, oracle, m, at_end, kind):
    """m = 11 (66 rows: the second pass of the matvec loop) and m = 43 (258 rows: two energy workgroups, c in the second), at
    the front and at the end of an m + 3 pose problem; H the marginal of a chain -- plain, under units(3), gauge-free.
    Stand-alone calls on WindowPrior.addr()."""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import WindowPrior
    n, rows = m + 3, 6 * m
    first = 3 if at_end else 0
    rng = np.random.default_rng([4, m, at_end])
    x0 = np.stack([oracle.pose_retract(I12, np.r_[0.5 * rng.uniform(-1, 1, 3), rng.normal(size=3)]) for _ in range(m)])
    poses = np.stack([oracle.pose_retract(I12, rng.normal(size=6)) for _ in range(n)])
    for i in range(m):
        poses[first + i] = oracle.pose_retract(x0[i], 0.03 * rng.normal(size=6))
    x = 0.02 * rng.normal(size=6 * n)
    new = np.stack([oracle.pose_retract(poses[k], x[6 * k:6 * k + 6]) for k in range(n)])
    H, g, c = fc.prior_of(rows, kind)
    ref = fl.Prior(first, x0, H, g, c)
    dl, dl_new = fl.delta(oracle, ref, poses), fl.delta(oracle, ref, new)
    assert 0.01 < np.abs(dl).max() < 0.2
    win = slice(6 * first, 6 * first + rows)
    grad_ref, e_ref, mag_grad, mag_e = fc.prior_energy_ref(H, g, c, dl)
    _, lin_ref, _, mag_lin = fc.prior_energy_ref(H, g, c, dl.astype(fc.LD) + x[win].astype(fc.LD))
    _, new_ref, _, mag_new = fc.prior_energy_ref(H, g, c, dl_new)
    numpy_values = (fl.system(oracle, ref, poses, n)[1][win], fl.error(oracle, ref, poses), fl.linear_error(oracle, ref, poses, x),
                    fl.error(oracle, ref, new))
    p, st, lib = _lib.ptr, _lib.current_stream_ptr(), _lib.load()
    d_poses, d_new, d_dp = dev(poses), dev(new), dev(x.reshape(n, 6))

    def run(scale):
        W = WindowPrior(first, x0, np.ldexp(H, scale), np.ldexp(g, scale), float(np.ldexp(c, scale)), n)
        work = torch.empty(int(lib.vus_window_prior_work_doubles(W.addr())), **F64)
        grad, err, err2, out = (torch.full((k,), float("nan"), **F64) for k in (rows, 1, 1, 2))
        _lib.call("vus_window_prior_linearize", W.addr(), p(d_poses), p(grad), p(err), p(work), st)
        _lib.call("vus_window_prior_error", W.addr(), p(d_poses), p(err2), p(work), st)
        _lib.call("vus_window_prior_eval_step", W.addr(), p(d_poses), p(d_dp), p(d_new), p(out), p(work), st)
        return W, grad, (grad.cpu().numpy(), err.cpu().numpy(), err2.cpu().numpy(), out.cpu().numpy())
    W, d_grad, base = run(0)
    tag = f"m={m} first={first} {kind}"
    assert np.array_equal(base[1], base[2])                  # the stand-alone error is the linearisation's
    _energy_line("window_prior", tag, ("grad", "error", "linear", "new"), (grad_ref, e_ref, lin_ref, new_ref),
                 (mag_grad, mag_e, mag_lin, mag_new), numpy_values, (base[0], base[1][0], base[3][0], base[3][1]))
    assert all(np.array_equal(a, b) for a, b in zip(base, run(0)[2]))                       # two runs: the same bits
    for scale in (200, -200):                               # only products and fixed-order sums: exact scaling
        scaled = run(scale)[2]
        exact = all(np.array_equal(np.ldexp(a, -scale), b) for a, b in zip(scaled, base))
        print(f"FLCOND\twindow_prior-scale\t{tag}\t{scale}\t{'bit-exact' if exact else 'differs'}")
        assert exact, (tag, scale)
    # assemble on a band pre-filled with random values
    band = m - 1 if not at_end else m + 2
    S0, g0 = rng.normal(size=(n, band + 1, 36)), rng.normal(size=(n, 6))
    d_S, d_gs = dev(S0), dev(g0)
    _lib.call("vus_window_prior_check", W.addr(), band, st)
    _lib.call("vus_window_prior_assemble", W.addr(), p(d_grad), band, p(d_S), p(d_gs), st)
    Hbig, gbig = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    Hbig[win, win] = H
    gbig[win] = base[0]
    inside_g = np.zeros(6 * n, bool)
    inside_g[win] = True
    _assemble_check(S0, g0.reshape(-1), d_S.cpu().numpy(), d_gs.cpu().numpy().reshape(-1), bc.dense_to_band(Hbig, band), gbig,
                    _window_mask(n, band, np.arange(6 * n)[win]), inside_g)


@pytest.mark.parametrize("kind", fc.PRIOR_KINDS)
@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("m", [5, 18])
def test_nav_window_prior_at_sizes_with_a_second_pass_and_a_second_energy_workgroup(gpu, oracle, m, at_end, kind):
    """m = 5 (75 rows: eleven columns of a second pass) and m = 18 (270 rows: five passes, two energy workgroups, c in the
    second), at the front and at the end of an m + 3 keyframe problem.  Stand-alone calls on NavWindowPrior.addr()."""
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import NavWindowPrior
    n, rows = m + 3, 15 * m
    nN = 3 * n
    first = 3 if at_end else 0
    rng = np.random.default_rng([5, m, at_end])
    x0 = np.stack([oracle.pose_retract(I12, np.r_[0.5 * rng.uniform(-1, 1, 3), rng.normal(size=3)]) for _ in range(m)])
    v0, b0 = rng.normal(size=(m, 3)), 0.1 * rng.normal(size=(m, 6))
    poses = np.stack([oracle.pose_retract(I12, rng.normal(size=6)) for _ in range(n)])
    vels, biases = rng.normal(size=(n, 3)), 0.1 * rng.normal(size=(n, 6))
    for i in range(m):
        poses[first + i] = oracle.pose_retract(x0[i], 0.03 * rng.normal(size=6))
        vels[first + i] = v0[i] + 0.03 * rng.normal(size=3)
        biases[first + i] = b0[i] + 0.03 * rng.normal(size=6)
    x = 0.02 * rng.normal(size=18 * n)                      # the padding coordinates too: the family must not read them
    npo, nv, nb = nbr.retract(oracle, poses, vels, biases, x)
    H, g, c = fc.prior_of(rows, kind)
    ref = fn.NavPrior(first, x0, v0, b0, H, g, c)
    dl, dl_new = fn.delta(oracle, ref, poses, vels, biases), fn.delta(oracle, ref, npo, nv, nb)
    assert 0.01 < np.abs(dl).max() < 0.2
    win = fn.rows(first, m)
    grad_ref, e_ref, mag_grad, mag_e = fc.prior_energy_ref(H, g, c, dl)
    _, lin_ref, _, mag_lin = fc.prior_energy_ref(H, g, c, dl.astype(fc.LD) + x[win].astype(fc.LD))
    _, new_ref, _, mag_new = fc.prior_energy_ref(H, g, c, dl_new)
    numpy_values = (fn.system(oracle, ref, poses, vels, biases, n)[1][win], fn.error(oracle, ref, poses, vels, biases),
                    fn.linear_error(oracle, ref, poses, vels, biases, x), fn.error(oracle, ref, npo, nv, nb))
    p, st, lib = _lib.ptr, _lib.current_stream_ptr(), _lib.load()
    state, new_state, d_dp = [dev(a) for a in (poses, vels, biases)], [dev(a) for a in (npo, nv, nb)], dev(x.reshape(nN, 6))

    def run(scale):
        W = NavWindowPrior(first, x0, v0, b0, np.ldexp(H, scale), np.ldexp(g, scale), float(np.ldexp(c, scale)), n)
        work = torch.empty(int(lib.vus_nav_window_prior_work_doubles(W.addr())), **F64)
        grad, err, err2, out = (torch.full((k,), float("nan"), **F64) for k in (rows, 1, 1, 2))
        _lib.call("vus_nav_window_prior_linearize", W.addr(), *map(p, state), p(grad), p(err), p(work), st)
        _lib.call("vus_nav_window_prior_error", W.addr(), *map(p, state), p(err2), p(work), st)
        _lib.call("vus_nav_window_prior_eval_step", W.addr(), *map(p, state), p(d_dp), *map(p, new_state), p(out), p(work), st)
        return W, grad, (grad.cpu().numpy(), err.cpu().numpy(), err2.cpu().numpy(), out.cpu().numpy())
    W, d_grad, base = run(0)
    tag = f"m={m} first={first} {kind}"
    assert np.array_equal(base[1], base[2])
    _energy_line("nav_window_prior", tag, ("grad", "error", "linear", "new"), (grad_ref, e_ref, lin_ref, new_ref),
                 (mag_grad, mag_e, mag_lin, mag_new), numpy_values, (base[0], base[1][0], base[3][0], base[3][1]))
    assert all(np.array_equal(a, b) for a, b in zip(base, run(0)[2]))
    for scale in (200, -200):
        scaled = run(scale)[2]
        exact = all(np.array_equal(np.ldexp(a, -scale), b) for a, b in zip(scaled, base))
        print(f"FLCOND\tnav_window_prior-scale\t{tag}\t{scale}\t{'bit-exact' if exact else 'differs'}")
        assert exact, (tag, scale)
    band = 3 * m - 1 if not at_end else 3 * m + 3
    S0, g0 = rng.normal(size=(nN, band + 1, 36)), rng.normal(size=(nN, 6))
    d_S, d_gs = dev(S0), dev(g0)
    _lib.call("vus_nav_window_prior_check", W.addr(), band, st)
    _lib.call("vus_nav_window_prior_assemble", W.addr(), p(d_grad), band, p(d_S), p(d_gs), st)
    Hbig, gbig = np.zeros((18 * n, 18 * n)), np.zeros(18 * n)
    Hbig[np.ix_(win, win)] = H
    gbig[win] = base[0]
    inside_g = np.zeros(18 * n, bool)
    inside_g[win] = True
    inside_S = _window_mask(nN, band, win)
    padS, padg = fc.nav_padding_masks(nN, band)
    assert not (inside_S & padS).any() and not (inside_g & padg.reshape(-1)).any()         # the padding lies outside: untouched
    _assemble_check(S0, g0.reshape(-1), d_S.cpu().numpy(), d_gs.cpu().numpy().reshape(-1), nbr.band_blocks(Hbig, nN, band), gbig,
                    inside_S, inside_g)
