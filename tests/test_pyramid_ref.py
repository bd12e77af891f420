"""The plain statements of tests/pyramid_ref.py against the oracle twins vus_resize_bilinear_cpu, vus_select_grid_cpu and
vus_pyramid_append_cpu on every case of the tables, and the tables' own coverage, shown with the statements alone: which
load path of the resize kernel a shape reaches, which cells a grid case leaves empty, truncates or cuts."""
import ctypes

import numpy as np
import pytest

import pyramid_ref as R
import track_ref


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ----------------------------------------------------------------------------------------------------------------------
# resize

@pytest.mark.parametrize("name", [c["name"] for c in R.RESIZE_CASES])
def test_resize_reference_equals_oracle(oracle, name):
    c, rows, want = R.resize_case(name)
    n, Hd, Wd, pd = c["n_img"], c["Hd"], c["Wd"], c["pitch_d"]
    src = np.ascontiguousarray(rows)
    out = np.full((n, Hd, pd), R.FILL, np.uint8)
    rc = oracle.lib().vus_resize_bilinear_cpu(_p(src), n, c["Hs"], c["Ws"], c["pitch_s"], _p(out), Hd, Wd, pd)
    assert rc == 0
    assert np.array_equal(out[:, :, :Wd], want)
    assert (out[:, :, Wd:] == R.FILL).all() and np.array_equal(src, rows)


def test_resize_reference_on_small_hand_cases():
    """Identity copies; x1/2 averages 2 x 2 blocks exactly (weights 1024 / 1024); one pixel from a constant is the constant."""
    img = np.random.default_rng(0).integers(0, 256, (2, 8, 12), dtype=np.uint8)
    assert np.array_equal(R.resize_bilinear(img, 2, 8, 12, 12, 8, 12), img)
    half = R.resize_bilinear(img, 2, 8, 12, 12, 4, 6)
    blocks = img.reshape(2, 4, 2, 6, 2).astype(np.int64).sum(axis=(2, 4))
    assert np.array_equal(half, (blocks * 1024 * 1024 + (1 << 21)) >> 22)
    i0, i1, w = R.resize_coeff(12, 6)
    assert (w == 1024).all() and np.array_equal(i0, np.arange(0, 12, 2)) and np.array_equal(i1, i0 + 1)
    i0, i1, w = R.resize_coeff(7, 30)                                        # up-scaling: the first centres lie left of pixel 0
    assert i0[0] == 0 and i1[0] == 0 and i0[-1] == 6 and i1[-1] == 6 and (0 <= w).all() and (w <= 2048).all()


def test_resize_table_reaches_both_load_paths_and_every_edge():
    cls = {c["name"]: R.resize_path_class(c["Ws"], c["Wd"]) for c in R.RESIZE_CASES}
    assert R.resize_path_class(100, 40) == "dword" and R.resize_path_class(100, 20) == "byte"
    assert R.resize_path_class(100, 29) == "mixed"
    assert {"dword", "byte", "mixed"} <= set(cls.values())
    # the five shapes of test_frontend_gpu.py::test_resize_bilinear_bit_exact never leave the dword path
    assert all(R.resize_path_class(ws, wd) == "dword" for ws, wd in ((56, 56), (56, 28), (1280, 1067), (357, 298), (53, 90)))
    for pat in R.PATTERNS:                                                 # every pixel pattern on every path class
        assert {cls[c["name"]] for c in R.RESIZE_CASES if c["pattern"] == pat} == {"dword", "byte", "mixed"}, pat
    C = R.RESIZE_CASES
    assert {c["Ws"] for c in C} >= {7, 11, 12, 13} and {c["Wd"] for c in C} >= {1, 2, 3, 4, 5, 255, 256, 257}
    assert {c["Hd"] for c in C} >= {1, 7, 8, 9} and {c["n_img"] for c in C} == {1, 3}
    assert {c["src_skew"] for c in C} == {0, 1, 2, 3} and {c["dst_skew"] for c in C} == {0, 1, 2, 3}
    for k in ("dword", "byte", "mixed"):
        assert any(c["pitch_s"] > c["Ws"] and cls[c["name"]] == k for c in C), k
        assert any(c["pitch_d"] > c["Wd"] and cls[c["name"]] == k for c in C), k
    assert any(c["Hd"] < c["Hs"] and c["Wd"] > c["Ws"] for c in C) and any(c["Hd"] > c["Hs"] and c["Wd"] < c["Ws"] for c in C)
    # the 32-bit edge: which strips 32-bit coefficients can serve
    fits = {c["name"]: R.fits_32_bits(c["Hs"], c["Hd"]) and R.fits_32_bits(c["Ws"], c["Wd"]) for c in C}
    wide = sorted(k for k, v in fits.items() if not v)
    assert wide == sorted(["strip_7x40000_to_7x33333", "strip_40000x7_to_33333x7", "strip_7x7_to_1x1048575",
                           "strip_7x7_to_1x1048577"])
    assert fits["strip_7x32768_to_7x27307"]


def _coeff_32_bits(Ns, Nd):
    """resize_coeff with every intermediate wrapped to 32 bits, as `int` / `unsigned` arithmetic would leave it: used only
    to show that the strips of the table are shapes at which 32 bits are NOT enough (and 32768 -> 27307 one at which they are)."""
    M = 1 << 32
    d = np.arange(Nd, dtype=np.int64)
    num = ((2 * d + 1) * Ns - Nd + (M >> 1)) % M - (M >> 1)
    den = 2 * Nd
    ix = np.where(num >= 0, num // den, -(((-num + den - 1) % M) // den))
    rem = (num - ix * den) % M
    w = ((rem * 2048 + Nd) % M) // den
    return np.clip(ix, 0, Ns - 1), np.clip(ix + 1, 0, Ns - 1), w


@pytest.mark.parametrize("Ns,Nd,n_wrong,first", [(40000, 33333, 6489, 26844), (36000, 30000, 173, 29827), (32768, 27307, 0, None),
                                                 (7, 2 ** 20 - 1, 254, 74862)])
def test_where_32_bit_coefficients_go_wrong(Ns, Nd, n_wrong, first):
    a, b = R.resize_coeff(Ns, Nd), _coeff_32_bits(Ns, Nd)
    bad = (a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2])
    assert int(bad.sum()) == n_wrong and (first is None or int(np.argmax(bad)) == first)
    assert R.fits_32_bits(Ns, Nd) == (n_wrong == 0)


# ----------------------------------------------------------------------------------------------------------------------
# grid selection

@pytest.mark.parametrize("name", list(R.GRID_CASES))
def test_select_grid_reference_equals_oracle(oracle, name):
    c = R.GRID_CASES[name]
    want, wc = R.grid_reference(name)
    got, gc = oracle.select_grid(c["keys"], c["count"], c["H"], c["W"], c["gr"], c["gc"], c["per"], c["max_kp"])
    assert np.array_equal(gc, wc) and np.array_equal(got, want)


def test_select_grid_reference_on_a_hand_case():
    """4 x 6 image, 2 x 3 cells of 2 x 2 pixels, 2 per cell."""
    k = lambda score, y, x: ((255 - score) << 24) | (y * 6 + x)
    keys = np.array([[k(10, 0, 0), k(30, 1, 1), k(20, 0, 1), k(20, 0, 1),                # cell 0: three keys, one twice
                      k(5, 3, 5), R.KEY_INVALID, k(200, 4, 0), k(7, 0, 4), k(7, 1, 5), k(7, 0, 5),   # (4, 0) is no pixel
                      k(255, 2, 2)]], np.uint32)                                          # beyond the count
    kp, cnt = R.select_grid(keys, [10], 11, 4, 6, 2, 3, 2, 8)
    assert cnt[0] == 5
    assert list(kp[0]) == [k(30, 1, 1), k(20, 0, 1), k(7, 0, 4), k(7, 0, 5), k(5, 3, 5), R.KEY_INVALID, R.KEY_INVALID, R.KEY_INVALID]
    kp, cnt = R.select_grid(keys, [10], 11, 4, 6, 2, 3, 2, 3)
    assert cnt[0] == 3 and list(kp[0]) == [k(30, 1, 1), k(20, 0, 1), k(7, 0, 4)]
    assert R.select_grid(keys, [-4], 11, 4, 6, 2, 3, 2, 3)[1][0] == 0
    assert k(255, 2, 2) in list(R.select_grid(keys, [99], 11, 4, 6, 2, 3, 2, 8)[0][0])    # clamped to cand_cap: slot 10 is read


def test_grid_table_contains_what_it_is_meant_to():
    facts = {n: R.grid_case_facts(n) for n in R.GRID_CASES}
    every = [(n, f, R.GRID_CASES[n]) for n, fs in facts.items() for f in fs]
    assert any((f["have"] == 0).any() and f["count"] > 0 for _, f, _ in every)                          # an empty cell
    assert any(((f["have"] > c["per"]) & (f["kept"] == c["per"])).any() for _, f, c in every)          # truncated by per_cell
    assert any(((f["kept"] > 0) & (f["kept"] < np.minimum(f["have"], c["per"]))).any() for _, f, c in every)   # cut by max_kp
    assert any(f["count"] == 0 for _, f, _ in every) and any(f["count"] == c["max_kp"] for _, f, c in every)
    assert any(f["count"] == c["gr"] * c["gc"] * c["per"] for _, f, c in every)                         # every cell full
    # the population case holds cells of 0, 1, per - 1, per and per + 1 keys
    c = R.GRID_CASES["populations_k48"]
    have = facts["populations_k48"][0]["have"]
    assert list(have) == c["pops"] and {0, 1, c["per"] - 1, c["per"], c["per"] + 1} <= set(have.tolist())
    cut = facts["populations_k6"][0]
    assert list(cut["kept"][:5]) == [0, 1, 3, 2, 0] and cut["count"] == 6
    assert [R.GRID_CASES[n]["max_kp"] for n in R.GRID_CASES if n.startswith("populations")] == [1, 3, 6, 33, 34, 48, 64]
    assert facts["populations_k34"][0]["count"] == 34 and facts["populations_k64"][0]["count"] == 34
    # counts: empty, negative, above cand_cap, around the workgroup
    L = R.GRID_CASES["lengths"]
    assert list(L["count"]) == [1023, 1024, 1025, 4099, 0, -3, L["cap"] + 5]
    assert [f["count"] for f in facts["lengths"]][4:6] == [0, 0] and facts["lengths"][6]["count"] > 0
    # the keys beyond the count would win: reading one slot too many changes the result
    for name in ("lengths", "grid1x1", "equal_scores"):                     # cases whose max_kp cuts no cell
        c = R.GRID_CASES[name]
        more = np.where((c["count"] >= 0) & (c["count"] < c["cap"]), c["count"] + 1, c["count"])
        kp, _ = R.select_grid(c["keys"], more, c["cap"], c["H"], c["W"], c["gr"], c["gc"], c["per"], c["max_kp"])
        changed = (kp != R.grid_reference(name)[0]).any(axis=1)
        assert changed[(c["count"] >= 0) & (c["count"] < c["cap"])].all(), name
    # bad keys inside the count; equal scores; cells without a pixel
    for name in ("lengths", "grid5x7_on_100x131", "one_column_256_rows"):
        c = R.GRID_CASES[name]
        k = c["keys"][0, :int(c["count"][0])].astype(np.int64)
        assert (k == R.KEY_INVALID).any() and ((k & R.POS_MASK) >= c["H"] * c["W"]).sum() > 1 and len(np.unique(k)) < len(k)
    c = R.GRID_CASES["equal_scores"]
    kp, cnt = R.grid_reference("equal_scores")
    assert cnt[0] == 48 and (kp[0] >> 24 == 200).all()
    c = R.GRID_CASES["more_rows_than_the_image"]
    rows_with_pixels = np.unique(np.arange(c["H"]) * c["gr"] // c["H"])
    assert len(rows_with_pixels) < c["gr"] and facts["more_rows_than_the_image"][0]["count"] > 0
    c = R.GRID_CASES["image_of_2p24_pixels"]
    kp, cnt = R.grid_reference("image_of_2p24_pixels")
    assert (kp[0, :cnt[0]] & R.POS_MASK == R.POS_MASK).sum() == 2 and (c["keys"][0, :200] == R.KEY_INVALID).any()   # the last pixel, twice


# ----------------------------------------------------------------------------------------------------------------------
# level merge

@pytest.mark.parametrize("nulls", R.APPEND_NULLS, ids=lambda v: "level%d_xy%d" % (not v[0], not v[1]))
@pytest.mark.parametrize("name", list(R.APPEND_CASES))
def test_pyramid_append_reference_equals_oracle_at_the_edges(oracle, name, nulls):
    c = R.APPEND_CASES[name]
    want = R.append_reference(name)
    got = R.append_entry(c)
    if nulls[0]:
        got["kp_level"] = None
    if nulls[1]:
        got["kp_xy_q4"] = None
    oracle.pyramid_append(c["keys"], c["lvl_count"], c["desc"], c["angle"], c["Hl"], c["Wl"], c["level"], c["H0"], c["W0"], got)
    for k, v in got.items():
        if v is not None:
            assert np.array_equal(v, want[k]), k


def test_append_table_contains_what_it_is_meant_to():
    c = R.APPEND_CASES["negative_and_overfull"]
    m = R.append_reference("negative_and_overfull")
    entry, asked, K = c["entry_count"], c["lvl_count"], c["max_kp"]
    assert (asked < 0).sum() >= 3 and ((asked < 0) & (entry == K)).any() and ((asked < 0) & (entry == 0)).any()
    assert ((entry == K) & (asked > 0)).any() and ((entry > K) & (asked > 0)).any() and ((entry > K) & (asked == 0)).any()
    assert (m["kp_count"] >= entry).all()                                   # the count never decreases
    untouched = (asked <= 0) | (entry >= K)
    fresh = R.append_entry(c)
    for k in ("kp_keys", "desc", "angle", "kp_level", "kp_xy_q4"):
        assert np.array_equal(m[k][untouched], fresh[k][untouched]), k
    assert (m["kp_count"][~untouched] > entry[~untouched]).all() and (~untouched).sum() >= 2
    c = R.APPEND_CASES["stride_level255_larger_level"]
    m = R.append_reference("stride_level255_larger_level")
    assert list(c["lvl_count"][:4]) == [255, 256, 257, 1000] and c["level"] == 255 and c["Wl"] > c["W0"] and c["Hl"] > c["H0"]
    assert list(m["kp_count"]) == [255, 259, 257, 1100, 1100, 1100] and (m["kp_level"][0, :255] == 255).all()
    for name in ("last_pixel_of_2p24_same_size", "last_pixel_of_2p24_smaller_level"):
        c, m = R.APPEND_CASES[name], R.append_reference(name)
        assert c["H0"] * c["W0"] == 1 << 24
        slot = int(c["entry_count"][0])
        assert m["kp_keys"][0, slot] == (7 << 24) | R.POS_MASK               # the last pixel of level 0, score byte kept
    assert track_ref.POS_MASK == R.POS_MASK
