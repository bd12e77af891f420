"""The harness of tests/test_closure_cond_gpu.py certified on the CPU (tests/closure_cond_ref.py): the keys cover what they
claim, every system has a reference, the low-rank algorithm in f64 LAPACK passes the bounds the kernels are held to where it
belongs to the accuracy family, at most one key in ten does not, every defect the bounds must see is seen on every shape,
and the bridge sweep (profiles/closure_conditioning.md holds its lines) shows where the low-rank path loses digits."""
import numpy as np
import pytest

import band_cond_ref as bc
import closure_cond_ref as cc


def test_keys_cover_the_layouts_weights_and_strides():
    ks = cc.keys()
    assert len(ks) == len(set(ks))
    for shape in cc.SHAPES:
        mine = [k for k in ks if k[:2] == shape and k[7] == 1]
        assert {k[5] for k in mine} == set(cc.LAYOUTS) and {k[6] for k in mine} == set(cc.GAMMAS)
        assert {(k[2], k[3], k[4]) for k in mine} == {k[2:] for k in bc.accuracy_keys([shape])}
        for layout in cc.LAYOUTS:
            assert len({k[6] for k in mine if k[5] == layout}) >= 2, (shape, layout)
    assert {k[7]: k[:2] for k in ks if k[7] > 1} == cc.STRIDE_KEYS


@pytest.mark.parametrize("n,band", cc.SHAPES)
def test_layouts_are_what_they_claim(n, band):
    for stride in [1] + [s for s, shape in cc.STRIDE_KEYS.items() if shape == (n, band)]:
        D = band // stride + 1
        seven = cc.layout_pairs("seven", n // stride, D)
        assert len(seven) == 7 and len(set(seven)) == 6                                   # two factors on one pair
        assert any((j, i) in seven for i, j in seven)                                     # one pair in both key orders
        assert any(i > j for i, j in seven) and any(i < j for i, j in seven)
        assert min(abs(i - j) for i, j in seven) == D                                     # exactly one pose outside the band
        assert max(np.bincount(np.ravel(seven))) >= 3                                     # factors sharing a node
        for layout, k in (("one", 1), ("k63", 63), ("k64", 64), ("same64", 64)):
            pairs = cc.layout_pairs(layout, n // stride, D)
            assert len(pairs) == k and all(0 <= min(p) and max(p) < n // stride and abs(p[0] - p[1]) >= D for p in pairs)
        assert len(set(cc.layout_pairs("same64", n // stride, D))) == 1
    s = cc.system(n, band, 1e-2, "all", 0, "seven", 1.0)
    for _, J1, J2, *_ in s.fac:
        assert np.array_equal(J2, np.triu(J2)) and np.linalg.cond(J2) <= 10.0 * (1 + 1e-12) and np.array_equal(J1, -J2)
    got = np.abs(cc.low_rank_term(s.U)).max() / np.abs(s.Bm).max()
    assert abs(float(got) - 1.0) <= 1e-12


def test_same_pair_capacitance_has_six_large_eigenvalues():
    s = cc.system(23, 7, 1e-2, "all", 0, "same64", 1e6)
    ev = np.linalg.eigvalsh(s.capacitance[1])
    assert (ev[-6:] > 1e3).all() and np.abs(ev[:-6] - 1.0).max() <= 1e-6 and s.m == 384


@pytest.mark.parametrize("n,band", cc.SHAPES)
def test_every_key_has_a_reference_and_the_accuracy_family_passes_its_bounds(n, band):
    """LAPACK factors every A and is backward stable on it; the refined reference of right-hand side 0, solved once more
    with exact residuals (System.certify of band_cond_ref), has a tenth of LAPACK's backward error or less (cond(A) reaches
    1e15 here, two decades beyond band_cond_ref's systems, and two exact steps no longer gain three decades) and lies within
    1 % of the forward bound it is used to check, so its own error cannot decide that check; the low-rank solve in f64
    passes the bounds wherever the family rule admits the key."""
    for key in cc.keys([(n, band)]):
        s = cc.system(*key)
        assert s.factored, s.name
        assert s.eta_direct.max() <= 4 * bc.EPS, (s.name, s.eta_direct.max())
        eta_ref, dist = s.certify(0)
        assert eta_ref <= 0.1 * s.eta_direct[0], (s.name, eta_ref, s.eta_direct[0])
        assert dist <= 0.01 * s.fwd_bound, (s.name, dist, s.fwd_bound)
        s.check(s.X_direct, "LAPACK on A")
        if s.accurate:
            s.check(s.X_wood, "low-rank solve in f64")
            assert s.fwd_wood.max() <= cc.FAMILY_RATIO * max(s.fwd_direct.max(), cc.FAMILY_FLOOR)


def test_at_most_one_key_in_ten_is_outside_the_accuracy_family():
    ks = cc.keys()
    loss = [f for f in map(cc.family, ks) if not f[1]]
    for name, _, ratio, fw, fd in loss:
        print(f"CCOND\tloss family\t{name}\t{fw:.2e}\t{fd:.2e}\t{ratio:.1f}")
    print(f"CCOND\tfamily split\t{len(ks) - len(loss)} accuracy\t{len(loss)} loss")
    assert 10 * len(loss) <= len(ks), (len(loss), len(ks))


@pytest.mark.parametrize("defect", list(cc.DEFECTS))
@pytest.mark.parametrize("n,band", cc.SHAPES)
def test_the_bounds_see_every_defect_on_every_shape(n, band, defect):
    """Z at 24 bits, C without + I, C from its (perturbed) upper triangle, a wrong sign on one right-hand side, U without
    the J2 block of its last factor: each fails check() on at least one accuracy-family key of the shape."""
    caught = []
    for key in cc.keys([(n, band)]):
        s = cc.system(*key)
        if s.accurate and not s.passes(s.defective(defect)):
            caught.append(s.name)
            break
    assert caught, (n, band, defect)


def test_an_independent_j1_holds_the_gauge_and_leaves_the_accuracy_family():
    """Why the synthetic factors are relative ones: on the chain with its prior on pose 0 only, a factor [J1 | J2] with an
    independent J1 also measures the motion common to all poses, cond(A) falls far below cond(B) and the low-rank solve,
    which goes through B, loses what the widened band keeps."""
    rel = cc.system(23, 7, 1e-5, "first", 0, "seven", 1.0)
    gen = cc.system(23, 7, 1e-5, "first", 0, "seven", 1.0, 1, False)
    print(f"CCOND\trelative factors\tloss ratio {rel.loss_ratio:.1f}\tindependent J1\t{gen.loss_ratio:.1f}")
    assert rel.accurate and not gen.accurate


# ---------------------------------------------------------------------------------------------- the bridge sweep
def test_bridge_family_is_the_chain_with_the_cut_factors_reweighted():
    n, band = 23, 7
    A = bc.system(n, band, 1e-2, "first").A
    assert np.array_equal(cc.bridged(A, n, band, 1.0), A)
    A0 = cc.bridged(A, n, band, 0.0)
    cut = 6 * (n // 2)
    assert not A0[cut:, :cut].any() and not A0[:cut, cut:].any()
    ev = np.linalg.eigvalsh(A0[cut:, cut:])                       # the far half floats: its six gauge motions are free
    assert np.abs(ev[:6]).max() <= 1e-12 * ev[-1] and ev[6] > 1e-6 * ev[-1]
    Ab = cc.bridged(A, n, band, 1e-4)
    assert np.linalg.eigvalsh(Ab).min() > 0 and np.array_equal(bc.band_to_dense(bc.dense_to_band(Ab, band)), Ab)


@pytest.mark.parametrize("n,band", cc.BRIDGE_SHAPES)
def test_bridge_sweep(n, band):
    """Prints the sweep.  Its claims: every bridged system has a reference; with the in-band link intact (beta = 1) every
    key is of the accuracy family; once the link is gone (beta = 0) the low-rank solve's error grows with 1 / lambda while
    the widened band's does not, and the smallest lambda leaves the accuracy family."""
    fw = {}
    for key in cc.bridge_keys([(n, band)]):
        s = cc.bridge(*key)
        assert s.factored, s.name
        print("CCOND\tbridge\t" + cc.bridge_line(s))
        if s.accurate:
            s.check(s.X_wood, "low-rank solve in f64")
        fw[key[2:]] = (s.fwd_wood.max(), s.fwd_direct.max(), s.accurate)
    for k in cc.BRIDGE_CLOSURES:
        assert all(fw[1.0, lam, k][2] for lam in cc.LAMBDAS)
        assert not fw[0.0, cc.LAMBDAS[-1], k][2]
        assert fw[0.0, 1e-11, k][0] > 1e3 * fw[0.0, 1e-3, k][0] and fw[0.0, 1e-11, k][1] < 1e3 * fw[0.0, 1e-3, k][1]
