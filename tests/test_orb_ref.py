"""tests/orb_ref.py pinned against the C oracle on the CPU: the plain statement of orientation + rBRIEF equals
vus_orient_rbrief_cpu on every generated case, angles and descriptors exactly; its derived tables equal the generated
header's; every case contains the edge it was generated for (asserted from the statement's own intermediate values);
and the known answers that follow from the tables alone hold."""
import numpy as np
import pytest

import orb_ref as R


def oracle_orient(oracle, img, blur, keys, counts, H, W):
    """vus_orient_rbrief_cpu with the image's own pitch and pre-filled outputs."""
    n, max_kp = keys.shape
    p = oracle._p
    img, blur = np.ascontiguousarray(img), np.ascontiguousarray(blur)
    keys, counts = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(counts, np.int32)
    desc = np.full((n, max_kp, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    ang = np.full((n, max_kp), 99, np.uint8)
    rc = oracle.lib().vus_orient_rbrief_cpu(p(img), p(blur), n, H, W, img.shape[2], p(keys), p(counts), max_kp, p(desc), p(ang))
    assert rc == 0
    return desc, ang


@pytest.mark.parametrize("name", R.image_case_names())
def test_statement_equals_oracle(oracle, name):
    img, blur, keys, counts, meta, ref = R.image_case(name)
    desc, ang = oracle_orient(oracle, img, blur, keys, counts, meta["H"], meta["W"])
    assert np.array_equal(ang, ref["angle"])
    assert np.array_equal(desc, ref["desc"])


def test_derived_tables_equal_the_header():
    assert np.array_equal(R.COS_Q14, R.header_array("VUS_ANGLE_COS"))
    assert np.array_equal(R.SIN_Q14, R.header_array("VUS_ANGLE_SIN"))
    assert np.array_equal(R.ROT, R.header_array("VUS_RBRIEF_ROT").reshape(30, 256, 4))
    assert np.array_equal(R.ROT[0], R.BASE) and np.abs(R.ROT).max() == R.REACH
    # the disc rebuilt from the half-widths is the header's, in its raster order
    assert np.array_equal(R.DISC_DX, R.header_array("VUS_DISC_DX")) and np.array_equal(R.DISC_DY, R.header_array("VUS_DISC_DY"))
    assert len(R.DISC_DX) == 749 and R.HALF_WIDTH[0] == R.RADIUS


def _maxima(m10, m01):
    pr = R.projections(m10, m01)
    return [np.flatnonzero(row == row.max()).tolist() for row in pr]


@pytest.mark.parametrize("name", ["ties", "ties_scaled"])
def test_tie_cases_contain_all_thirty_ties(name):
    """Exactly two maximal projections at every tie, and they are the intended adjacent pair; a unique maximum one unit
    to either side, on different sides; the moments are the prescribed ones; the first bin is the answer."""
    _, _, _, counts, meta, ref = R.image_case("moments:" + name)
    c = int(counts[0])
    assert c == 90 and [tuple(s[:2]) for s in meta["specs"]] == list(zip(ref["m10"][0, :c].tolist(), ref["m01"][0, :c].tolist()))
    mx = _maxima(ref["m10"][0, :c], ref["m01"][0, :c])
    pairs = set()
    for k in range(R.N_BINS):
        below, tie, above = mx[3 * k:3 * k + 3]
        k2 = (k + 1) % R.N_BINS
        assert sorted(tie) == sorted([k, k2]) and meta["roles"][3 * k + 1] == (k, "tie")
        assert ref["angle"][0, 3 * k + 1] == min(k, k2)                      # the first maximum: bin 0 for the pair 29 / 0
        assert len(below) == 1 and len(above) == 1 and below != above
        if name == "ties_scaled":
            assert below == [k] and above == [k2]
        else:
            assert max(abs(v) for v in meta["specs"][3 * k + 1][:2]) <= 2966
        pairs.add((k, k2))
    assert len(pairs) == 30
    assert tuple(meta["specs"][1][:2]) == (1703, 179) or name != "ties"      # bins 0 / 1, from the Q14 tables by hand
    assert tuple(meta["specs"][3 * 7 + 1][:2]) == (0, 1) or name != "ties"


def test_tie_slots_case_puts_ties_at_slot_0_slot_7_and_a_lone_live_slot():
    _, _, keys, counts, meta, ref = R.image_case("moments:tie_slots")
    c = int(counts[0])
    mx = _maxima(ref["m10"][0, :c], ref["m01"][0, :c])
    assert c == 17 and keys.shape[1] == 24 and c % 8 == 1                     # slot 16 is the only live one of its wave
    assert [j for j in range(c) if len(mx[j]) == 2] == [0, 7, 16]
    assert [sorted(mx[j]) for j in (0, 7, 16)] == [[3, 4], [0, 29], [7, 8]]   # pairs that straddle groups of four bins
    assert ref["angle"][0, [0, 7, 16]].tolist() == [3, 0, 7]


def test_flat_axes_and_sweep_case():
    """Known answers: a flat patch (0, 1 or 255) has zero moments and bin 0; the four axis directions at the largest
    moment a row or column carries; the sweep lands in every bin."""
    _, _, _, _, meta, ref = R.image_case("moments:flat_axes_sweep")
    roles = meta["roles"]
    flat = [j for j, r in enumerate(roles) if r[0] == "flat"]
    assert len(flat) == 3 and (ref["m10"][0, flat] == 0).all() and (ref["m01"][0, flat] == 0).all()
    assert (ref["angle"][0, flat] == 0).all()
    assert all(len(m) == 30 for m in _maxima(ref["m10"][0, flat], ref["m01"][0, flat]))     # all 30 projections equal
    axis = [j for j, r in enumerate(roles) if r[0] == "axis"]
    A = R.MOMENT_AXIS_MAX
    assert list(zip(ref["m10"][0, axis].tolist(), ref["m01"][0, axis].tolist())) == [(A, 0), (0, A), (-A, 0), (0, -A)]
    assert ref["angle"][0, axis].tolist() == [0, 7, 15, 22]                  # 90 degrees ties bins 7 / 8, 270 ties 22 / 23
    sweep = [j for j, r in enumerate(roles) if r[0] == "sweep"]
    assert ref["angle"][0, sweep].tolist() == list(range(30))


def test_saturated_case_reaches_the_largest_moments():
    """Per direction u, no image can give a larger m . u than 255 * sum over the disc of max(0, d . u); the case must
    reach 90 % of it (a condition on the generator).  The all-255 image has zero moments wherever the keypoint sits."""
    _, _, _, _, meta, ref = R.image_case("saturated")
    for j, (ux, uy) in enumerate(meta["dirs"]):
        bound = 255 * np.maximum(0, R.DISC_DX * ux + R.DISC_DY * uy).sum()
        got = ref["m10"][0, j] * ux + ref["m01"][0, j] * uy
        assert 0.9 * bound <= got <= bound, (j, got, bound)
    axis_bound = 255 * np.maximum(0, R.DISC_DX).sum()
    assert np.abs(ref["m10"][0]).max() >= 0.9 * axis_bound and np.abs(ref["m01"][0]).max() >= 0.9 * axis_bound
    assert axis_bound > 2 ** 16                                              # beyond what a 16-bit sum would hold
    assert (ref["m10"][1] == 0).all() and (ref["m01"][1] == 0).all() and (ref["angle"][1] == 0).all()


@pytest.mark.parametrize("complement", [False, True])
def test_impulse_case_descriptors_are_what_the_table_dictates(complement):
    """The expected bit sets come from the rotated table alone (orb_ref.impulse_expected_bits); the statement must give
    them.  Every bin, at least 16 offsets each, the extreme offsets of the bin's table among them."""
    _, _, _, _, meta, ref = R.image_case("impulse_complement" if complement else "impulse")
    assert (ref["angle"] == np.arange(30, dtype=np.uint8)[:, None]).all()
    assert np.array_equal(ref["desc"], meta["expected"])
    bits = np.unpackbits(meta["expected"].view(np.uint8), axis=-1)
    assert (bits.reshape(30, R.IMP_PER_BIN, -1).sum(-1) >= 1).all()           # non-empty, every one
    assert R.IMP_PER_BIN >= 16
    for k in range(30):
        assert not np.array_equal(meta["expected"][k], meta["expected"][(k + 1) % 30])
        pts = R.ROT[k][:, 0:2] if complement else R.ROT[k][:, 2:4]
        off = meta["offsets"][k]
        assert len({tuple(o) for o in off.tolist()}) == R.IMP_PER_BIN
        for axis in (0, 1):
            assert off[:, axis].max() == pts[:, axis].max() and off[:, axis].min() == pts[:, axis].min()
    assert np.abs(meta["offsets"]).max() == R.REACH


def test_equal_planes_case():
    """Known answer: a flat smoothed plane gives all-zero words.  The two-level and ramp planes decide many tests by
    equality (a == b, bit 0) and are not trivial."""
    _, blur, keys, counts, meta, ref = R.image_case("equal_planes")
    H, W = meta["H"], meta["W"]
    for i, name in enumerate(meta["planes"]):
        if name.startswith("const"):
            assert (blur[i] == blur[i, 0, 0]).all() and (ref["desc"][i] == 0).all()
            continue
        pos = keys[i].astype(np.int64) & R.KEY_POS_MASK
        y, x = pos // W, pos % W
        pat = R.ROT[ref["angle"][i]]
        a = blur[i][np.clip(y[:, None] + pat[:, :, 1], 0, H - 1), np.clip(x[:, None] + pat[:, :, 0], 0, W - 1)]
        b = blur[i][np.clip(y[:, None] + pat[:, :, 3], 0, H - 1), np.clip(x[:, None] + pat[:, :, 2], 0, W - 1)]
        assert (a == b).mean() > 0.05 and (a < b).mean() > 0.05 and (a > b).mean() > 0.05, name


def _sides(H, W, loader):
    pos = np.arange(H * W)
    return R.fast_path_conditions(pos // W, pos % W, H, W, loader)


def _layout_of(W, pitch, H):
    return "row_major" if (W | pitch | (H * pitch)) % 4 == 0 else "exact"


def _check_straddle(H, W, layout):
    """For each loader of the layout whose patch fits the image: keypoints that pass all four fast-path conditions, and
    for each condition keypoints that fail it alone.  A loader whose patch does not fit: none on the fast path."""
    for loader in R.LOADERS[layout]:
        Rr, DW, _ = loader
        c = _sides(H, W, loader)
        if H >= 2 * Rr + 1 and W >= 4 * DW:
            assert c.all(0).any(), (H, W, loader)
            for i in range(4):
                assert (~c[i] & np.delete(c, i, 0).all(0)).any(), (H, W, loader, i)
        else:
            assert not c.all(0).any(), (H, W, loader)


@pytest.mark.parametrize("H,W,pitch", R.EVERY_PIXEL_SHAPES)
def test_every_pixel_shapes_sit_on_both_sides_of_the_fast_path(H, W, pitch):
    layout = _layout_of(W, pitch, H)
    assert layout == ("exact" if (W % 2 or pitch in (67, 66)) else "row_major")
    _check_straddle(H, W, layout)
    if (H, W) == (20, 20):
        for lay in R.LOADERS:
            assert not any(_sides(H, W, ld).all(0).any() for ld in R.LOADERS[lay])
    for order in ("raster", "shuffled"):
        _, _, keys, counts, _, _ = R.image_case(f"every_pixel:{H}x{W}p{pitch}:{order}")
        assert counts[0] == H * W == keys.shape[1]
        assert np.array_equal(np.sort(keys[0] & R.KEY_POS_MASK), np.arange(H * W))    # every pixel, once
        assert len(np.unique(keys[0] >> 24)) > 100                                     # arbitrary top bits


@pytest.mark.parametrize("H,W,pitch", R.EVERY_PIXEL_TILED_SHAPES)
def test_tiled_shapes_sit_on_both_sides_of_the_fast_path(H, W, pitch):
    assert W % 16 == 0 and H % 8 == 0 and pitch == W and (H, W, pitch) in R.EVERY_PIXEL_SHAPES
    _check_straddle(H, W, "tiled")


def test_counts_cases_cover_every_count():
    seen = {k: set() for k in R.COUNTS_MAX_KP}
    for n in R.COUNTS_N_IMG:
        for k in R.COUNTS_MAX_KP:
            _, _, keys, counts, _, ref = R.image_case(f"counts:{n}:{k}")
            assert keys.shape == (n, k) and set(counts.tolist()) <= set(R.count_choices(k))
            seen[k] |= set(counts.tolist())
            for i in range(n):
                c = R.live_count(counts[i], k)
                assert (keys[i, c:] == R.KEY_INVALID).all() and (ref["desc"][i, c:] == 0).all() and (ref["angle"][i, c:] == 0).all()
    for k in R.COUNTS_MAX_KP:
        assert seen[k] == set(R.count_choices(k))


def test_top_key_bits_are_ignored():
    img, blur, keys, counts, meta, ref = R.image_case("every_pixel:40x44p44:shuffled")
    other = R.orient_rbrief(img, blur, keys & np.uint32(R.KEY_POS_MASK), counts, meta["H"], meta["W"])
    assert np.array_equal(other["desc"], ref["desc"]) and np.array_equal(other["angle"], ref["angle"])


@pytest.mark.parametrize("name", R.ORDER_CASES)
def test_order_cases_and_the_order_predicate(name):
    """The cases hold what they are named for; the predicate accepts the identity only where the keys are already grouped,
    accepts a by-cell sort, and refuses a moved unused slot, a repeated slot and an ungrouped order."""
    _, _, keys, counts, meta = R.order_case(name)
    H, W, max_kp = meta["H"], meta["W"], meta["max_kp"]
    n = keys.shape[0]
    assert keys.shape[1] == max_kp
    cw, ch = -(-W // R.CELL), -(-H // R.CELL)
    assert meta["refused"] == (cw * ch > R.MAX_CELLS)
    if name == "cells_1024":
        assert cw * ch == R.MAX_CELLS
    pos = keys.astype(np.int64) & R.KEY_POS_MASK
    cell = (pos // W // R.CELL) * cw + (pos % W) // R.CELL
    good = np.tile(np.arange(max_kp), (n, 1))
    for i in range(n):
        c = R.live_count(counts[i], max_kp)
        good[i, :c] = np.argsort(cell[i, :c], kind="stable")
    assert R.reference_order_is_valid(good, keys, counts, H, W)
    if name == "one_cell":
        assert all(len(np.unique(cell[i, :counts[i]])) == 1 for i in range(n))
        assert R.reference_order_is_valid(np.tile(np.arange(max_kp), (n, 1)), keys, counts, H, W)
    if name == "one_per_cell":
        assert sorted(cell[0].tolist()) == list(range(cw * ch))
    if name in ("count_full", "max_kp_8192", "odd_width", "cells_1024"):
        assert counts[0] == max_kp and not R.reference_order_is_valid(np.tile(np.arange(max_kp), (n, 1)), keys, counts, H, W)
        bad = good.copy()
        bad[0, 1] = bad[0, 0]                                    # a repeated slot
        assert not R.reference_order_is_valid(bad, keys, counts, H, W)
    if name == "small_max_kp":
        bad = good.copy()
        bad[1, [5, 6]] = bad[1, [6, 5]]                          # unused slots moved
        assert counts[1] == 5 and not R.reference_order_is_valid(bad, keys, counts, H, W)
    if name == "count0":
        assert np.array_equal(good, np.tile(np.arange(max_kp), (n, 1)))
    if name == "odd_width":
        assert W % R.CELL != 0
