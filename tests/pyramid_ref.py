"""Plain statements of vus_resize_bilinear and vus_select_grid (include/vus.h), written from the header's text with
Python integers and numpy int64 -- no 32-bit arithmetic, no code shared with the oracle or the kernels -- and the case
tables that tests/test_pyramid_ref.py (CPU, against the oracle twins) and tests/test_pyramid_gpu.py (the HIP kernels) both
run.  The level merge's statement is track_ref.pyramid_append; its edge cases are APPEND_CASES below."""
import functools

import numpy as np

import track_ref

KEY_INVALID = 0xFFFFFFFF
POS_MASK = 0x00FFFFFF


# ======================================================================================================================
# vus_resize_bilinear

def resize_coeff(Ns, Nd):
    """(i0, i1, w) int64 [Nd] of one axis: num = (2 d + 1) Ns - Nd, den = 2 Nd, ix = floor(num / den),
    w = round-half-up(2048 (num - ix den) / den), source indices clamp(ix), clamp(ix + 1)."""
    d = np.arange(Nd, dtype=np.int64)
    num = (2 * d + 1) * Ns - Nd
    den = 2 * Nd
    ix = num // den                                      # numpy's // floors, also below zero
    rem = num - ix * den
    w = (2 * 2048 * rem + den) // (2 * den)              # floor(2048 rem / den + 1/2)
    return np.clip(ix, 0, Ns - 1), np.clip(ix + 1, 0, Ns - 1), w


def resize_bilinear(buf, n_img, Hs, Ws, pitch_s, Hd, Wd):
    """buf: uint8, n_img images of Hs rows of pitch_s bytes (the first Ws of a row are pixels) -> uint8 [n_img, Hd, Wd]."""
    src = np.asarray(buf, np.uint8).reshape(-1)[:n_img * Hs * pitch_s].reshape(n_img, Hs, pitch_s)[:, :, :Ws].astype(np.int64)
    y0, y1, wy = resize_coeff(Hs, Hd)
    x0, x1, wx = resize_coeff(Ws, Wd)
    a, b = src[:, y0, :], src[:, y1, :]
    top = (2048 - wx) * a[:, :, x0] + wx * a[:, :, x1]
    bot = (2048 - wx) * b[:, :, x0] + wx * b[:, :, x1]
    out = ((2048 - wy)[None, :, None] * top + wy[None, :, None] * bot + (1 << 21)) >> 22
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_thread_paths(Ws, Wd):
    """bool [ceil(Wd / 4)]: True where the kernel's thread for destination columns 4t .. 4t+3 fetches three dwords per
    source row, False where it loads bytes.  This restates the kernel's SCHEDULE (csrc/pyramid.hip: Ws >= 12 and
    x1[3] - start < 12 with start = max(min(x0[0], Ws - 12), 0)), not the contract: the result does not depend on it.
    The tests use it to say which of the two load paths a shape reaches."""
    x0, x1, _ = resize_coeff(Ws, Wd)
    t = np.arange(-(-Wd // 4), dtype=np.int64)
    first, last = np.minimum(4 * t, Wd - 1), np.minimum(4 * t + 3, Wd - 1)
    start = np.maximum(np.minimum(x0[first], Ws - 12), 0)
    return (x1[last] - start < 12) & (Ws >= 12)


def resize_path_class(Ws, Wd):
    p = resize_thread_paths(Ws, Wd)
    return "dword" if p.all() else ("byte" if not p.any() else "mixed")


def fits_32_bits(Ns, Nd):
    """The 32-bit coefficient arithmetic of the kernel is exact on this axis (a schedule, as above): the largest
    numerator, the negative one's rounding term and rem * 2048 + Nd all stay inside 32 bits."""
    return (2 * Nd - 1) * Ns + Nd < 2 ** 31 and 4097 * Nd < 2 ** 32


FILL = 0xA5                       # what the destination buffer and the bytes around both buffers hold before the call
PATTERNS = ("random", "all255", "all0", "checker")


def _resize_case(name, i, Hs, Ws, Hd, Wd, pattern=None, plain=False):
    """plain: one image, tight pitches, aligned buffers (the large strips).  Otherwise pitch, alignment, image count and
    pixel pattern cycle with the case index i, so that every combination is met somewhere in the table."""
    if plain:
        n_img, ps, pd, ss, ds = 1, Ws, Wd, 0, 0
    else:
        n_img = 3 if i % 3 == 0 else 1
        ps = Ws + (0, 5, 1, 19)[i % 4]
        pd = Wd + (0, 3, 7, 1)[(i // 2) % 4]
        ss, ds = ((0, 0), (1, 0), (0, 1), (2, 3), (3, 2), (1, 1), (0, 2), (3, 0))[i % 8]
    return dict(name=name, n_img=n_img, Hs=Hs, Ws=Ws, pitch_s=ps, Hd=Hd, Wd=Wd, pitch_d=pd, src_skew=ss, dst_skew=ds,
                pattern=pattern or PATTERNS[0 if plain else (i // 3) % 4], seed=1000 + i)


def _resize_table():
    # per axis (source, destination): identity, x1/1.2, x1/2, 2.5, 3.45, 3.7 and 5 (the dword window holds 12 source
    # bytes: 2.5 stays inside it, 5 never does, 3.45 and 3.7 do for some threads), 60, 300, and up-scaling x1.7, x4.3
    scales = [(100, 100), (100, 83), (100, 50), (100, 40), (100, 29), (100, 27), (100, 20), (300, 5), (300, 1), (100, 170),
              (7, 30)]
    shapes = []
    for k, (ws, wd) in enumerate(scales):                      # columns take class k, rows another class
        hs, hd = scales[(k + 4) % len(scales)]
        shapes.append((hs, ws, hd, wd))
    shapes += [(100, 7, 50, 30), (7, 100, 30, 50),             # rows shrink while columns grow, and the reverse
               (9, 100, 9, 40), (9, 100, 9, 29), (9, 100, 9, 20)]
    shapes += [(8, w, 8, w - 2) for w in (7, 11, 12, 13)] + [(8, w, 5, 2 * w + 1) for w in (7, 11, 12, 13)]
    shapes += [(9, 13, 7, wd) for wd in (1, 2, 3, 4, 5)] + [(9, 300, 9, wd) for wd in (255, 256, 257)]
    shapes += [(20, 40, hd, 33) for hd in (1, 7, 8, 9)]
    cases = [_resize_case("%dx%d_to_%dx%d" % s, i, *s) for i, s in enumerate(shapes)]
    i = len(cases)
    for wd in (40, 29, 20):                                    # all-dword, mixed and all-byte columns on every pattern
        for pat in PATTERNS[1:]:
            cases.append(_resize_case("9x100_to_11x%d_%s" % (wd, pat), i, 9, 100, 11, wd, pattern=pat))
            i += 1
    # where 32-bit coefficients end: the two strips need 64 bits, 32768 -> 27307 is exact in 32; 7 -> 2^20 - 1 is the
    # last width whose rem * 2048 + Nd is below 2^32 only if rem stays small, 2^20 + 1 the first that needs 64 bits anyway
    for s in ((7, 40000, 7, 33333), (40000, 7, 33333, 7), (7, 32768, 7, 27307), (7, 7, 1, 2 ** 20 - 1), (7, 7, 1, 2 ** 20 + 1)):
        cases.append(_resize_case("strip_%dx%d_to_%dx%d" % s, i, *s, plain=True))
        i += 1
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


RESIZE_CASES = _resize_table()


def resize_pixels(c):
    """uint8 [n_img, Hs, Ws] of a case."""
    shape = (c["n_img"], c["Hs"], c["Ws"])
    if c["pattern"] == "random":
        return np.random.default_rng(c["seed"]).integers(0, 256, shape, dtype=np.uint8)
    if c["pattern"] == "checker":
        n, y, x = np.indices(shape)
        return (((n + y + x) & 1) * 255).astype(np.uint8)
    return np.full(shape, 255 if c["pattern"] == "all255" else 0, np.uint8)


@functools.lru_cache(maxsize=None)
def _resize_built(name):
    c = next(c for c in RESIZE_CASES if c["name"] == name)
    px = resize_pixels(c)
    n, Hs, Ws, ps = c["n_img"], c["Hs"], c["Ws"], c["pitch_s"]
    rows = np.empty((n, Hs, ps), np.uint8)
    rows[:, :, :Ws] = px
    rows[:, :, Ws:] = px[:, :, -1:] ^ 0xFF                 # padding: as far from the clamped edge pixel as a byte can be
    want = resize_bilinear(rows, n, Hs, Ws, ps, c["Hd"], c["Wd"])
    if c["pattern"] in ("all255", "all0"):
        assert (want == px[0, 0, 0]).all()
    rows.setflags(write=False)
    want.setflags(write=False)
    return rows, want


def resize_case(name):
    """(case dict, source rows uint8 [n_img, Hs, pitch_s] with poisoned padding, expected uint8 [n_img, Hd, Wd]); built
    once, read-only."""
    c = next(c for c in RESIZE_CASES if c["name"] == name)
    return (c,) + _resize_built(name)


# ======================================================================================================================
# vus_select_grid

def select_grid(keys, count, cand_cap, H, W, grid_row, grid_col, per_cell, max_kp):
    """keys uint32 [n_img, cand_cap], count [n_img] -> (kp_keys uint32 [n_img, max_kp], kp_count int32 [n_img]).
    The candidates of an image are its first min(max(count, 0), cand_cap) keys; VUS_KEY_INVALID and a key whose position
    is not a pixel of the image belong to no cell; the cell of pixel (y, x) is (y grid_row / H, x grid_col / W); every cell
    keeps its per_cell smallest DISTINCT keys, ascending; cells in row-major order, packed from slot 0, at most max_kp."""
    keys = np.asarray(keys, np.uint32).reshape(-1, cand_cap)
    n_img = keys.shape[0]
    out = np.full((n_img, max_kp), KEY_INVALID, np.uint32)
    cnt = np.zeros(n_img, np.int32)
    for n in range(n_img):
        c = min(max(int(count[n]), 0), cand_cap)
        cells = {}
        for k in {int(v) for v in keys[n, :c]}:
            pos = k & POS_MASK
            if k == KEY_INVALID or pos >= H * W:
                continue
            y, x = divmod(pos, W)
            cells.setdefault((y * grid_row // H, x * grid_col // W), set()).add(k)
        kept = []
        for cell in sorted(cells):
            kept += sorted(cells[cell])[:per_cell]
        kept = kept[:max_kp]
        out[n, :len(kept)] = kept
        cnt[n] = len(kept)
    return out, cnt


def cell_of(pos, H, W, gr, gc):
    return (pos // W) * gr // H * gc + (pos % W) * gc // W


def _positions_in_cell(rng, H, W, gr, gc, cell, k):
    pos = np.arange(H * W, dtype=np.int64)
    inside = pos[cell_of(pos, H, W, gr, gc) == cell]
    return rng.choice(inside, size=k, replace=False)


def _winners(rng, H, W, shape):
    """Keys of score 255 (the smallest score byte) at random pixels: they would be selected if they were read."""
    return rng.integers(0, H * W, shape).astype(np.uint32)


def _random_grid_case(name, seed, n_img, H, W, gr, gc, per, max_kp, cap, counts, scores=(0, 256), bad=True):
    """Random candidates; inside the count a sprinkling of duplicates, VUS_KEY_INVALID and positions beyond the image;
    beyond the count, keys that would win."""
    rng = np.random.default_rng(seed)
    keys = ((rng.integers(scores[0], scores[1], (n_img, cap)).astype(np.uint32) << 24) |
            rng.integers(0, H * W, (n_img, cap)).astype(np.uint32))
    counts = np.asarray(counts, np.int32)
    assert counts.shape == (n_img,)
    for n in range(n_img):
        c = min(max(int(counts[n]), 0), cap)
        if bad and c >= 8:
            m = max(c // 8, 1)
            keys[n, rng.integers(0, c, m)] = keys[n, rng.integers(0, c, m)]                       # duplicates
            keys[n, rng.integers(0, c, m)] = KEY_INVALID
            if H * W < POS_MASK:                                                                   # not a pixel
                keys[n, rng.integers(0, c, m)] = ((rng.integers(0, 4, m).astype(np.uint32) << 24) |
                                                  rng.integers(H * W, POS_MASK + 1, m).astype(np.uint32))
                keys[n, rng.integers(0, c)] = np.uint32(H * W)                                     # the first one past the image
                keys[n, rng.integers(0, c)] = np.uint32(POS_MASK)                                  # the last position a key can name
        keys[n, c:] = _winners(rng, H, W, cap - c)
    return dict(name=name, H=H, W=W, gr=gr, gc=gc, per=per, max_kp=max_kp, cap=cap, keys=keys, count=counts)


def _population_keys():
    """60 x 80, 3 x 4 cells, 4 per cell: cells holding 0, 1, per_cell - 1, per_cell, per_cell + 1 and more keys."""
    H, W, gr, gc, per = 60, 80, 3, 4, 4
    pops = [0, 1, 3, 4, 5, 9, 4, 0, 2, 5, 4, 6]
    rng = np.random.default_rng(77)
    keys = []
    for cell, k in enumerate(pops):
        pos = _positions_in_cell(rng, H, W, gr, gc, cell, k)
        keys += list((rng.integers(0, 256, k).astype(np.uint32) << 24) | pos.astype(np.uint32))
    keys = np.array(keys, np.uint32)
    rng.shuffle(keys)
    cap = len(keys) + 9
    row = np.concatenate([keys, _winners(rng, H, W, 9)])
    return H, W, gr, gc, per, pops, cap, row


def _grid_table():
    cases = []
    H, W, gr, gc, per, pops, cap, row = _population_keys()
    kept = sum(min(p, per) for p in pops)                        # 34
    # max_kp: 1; below per_cell; 6 cuts cell 3 after two of its four; one short of and exactly what the cells keep; the
    # grid's capacity; above it
    for K in (1, 3, 6, kept - 1, kept, gr * gc * per, gr * gc * per + 16):
        cases.append(dict(name="populations_k%d" % K, H=H, W=W, gr=gr, gc=gc, per=per, max_kp=K, cap=cap, keys=row[None].copy(),
                          count=np.array([len(row) - 9], np.int32), pops=pops))
    # list lengths around the 1024-thread workgroup, an empty, a negative and an over-long count (clamped to cand_cap);
    # H and W no multiples of the grid
    cap = 4104
    cases.append(_random_grid_case("lengths", 1, 7, 97, 131, 3, 4, 4, 64, cap, [1023, 1024, 1025, 4099, 0, -3, cap + 5]))
    cases.append(_random_grid_case("grid1x1", 2, 3, 33, 47, 1, 1, 6, 6, 300, [300, 5, 6]))
    # every pixel its own cell; few distinct scores, so a pixel is named by several keys and by duplicates
    cases.append(_random_grid_case("grid7x7_on_7x7", 3, 2, 7, 7, 7, 7, 2, 98, 400, [400, 37], scores=(250, 256)))
    cases.append(_random_grid_case("grid5x7_on_100x131", 4, 2, 100, 131, 5, 7, 3, 50, 700, [600, 90]))
    cases.append(_random_grid_case("grid256x256_on_300x300", 5, 1, 300, 300, 256, 256, 1, 300, 200, [150]))
    cases.append(_random_grid_case("more_rows_than_the_image", 6, 2, 7, 40, 16, 3, 2, 40, 200, [190, 200]))
    # one column of 300 pixels under 256 cell rows: the row index of a position beyond the image is as large as it gets
    cases.append(_random_grid_case("one_column_256_rows", 7, 2, 300, 1, 256, 1, 1, 300, 500, [500, 300]))
    # one score everywhere: the position decides
    cases.append(_random_grid_case("equal_scores", 8, 2, 50, 70, 3, 4, 4, 48, 300, [300, 299], scores=(200, 201)))
    # H W = 2^24: the position field of VUS_KEY_INVALID is the last pixel; a valid key names that pixel too
    c = _random_grid_case("image_of_2p24_pixels", 9, 1, 4096, 4096, 3, 4, 4, 48, 200, [200])
    c["keys"][0, 5] = np.uint32((1 << 24) | POS_MASK)
    c["keys"][0, 6] = np.uint32(POS_MASK)
    cases.append(c)
    cases.append(_random_grid_case("batch33", 10, 33, 60, 80, 3, 4, 4, 20, 256, [(37 * n) % 260 - 2 for n in range(33)]))
    for c in cases:
        c["keys"].setflags(write=False)
        c["count"].setflags(write=False)
    return {c["name"]: c for c in cases}


GRID_CASES = _grid_table()


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    c = GRID_CASES[name]
    kp, cnt = select_grid(c["keys"], c["count"], c["cap"], c["H"], c["W"], c["gr"], c["gc"], c["per"], c["max_kp"])
    kp.setflags(write=False)
    cnt.setflags(write=False)
    return kp, cnt


def grid_case_facts(name):
    """What a case's reference output contains, per image: valid candidates per cell, kept keys per cell."""
    c = GRID_CASES[name]
    kp, cnt = grid_reference(name)
    H, W, gr, gc = c["H"], c["W"], c["gr"], c["gc"]
    facts = []
    for n in range(kp.shape[0]):
        m = min(max(int(c["count"][n]), 0), c["cap"])
        cand = np.unique(c["keys"][n, :m]).astype(np.int64)
        cand = cand[(cand != KEY_INVALID) & ((cand & POS_MASK) < H * W)]
        have = np.bincount(cell_of(cand & POS_MASK, H, W, gr, gc), minlength=gr * gc)
        kept = np.bincount(cell_of(kp[n, :cnt[n]].astype(np.int64) & POS_MASK, H, W, gr, gc), minlength=gr * gc)
        facts.append(dict(have=have, kept=kept, count=int(cnt[n])))
    return facts


# ======================================================================================================================
# vus_pyramid_append at its edges (the statement is track_ref.pyramid_append)

def _append_case(name, seed, lvl_max_kp, max_kp, Hl, Wl, level, H0, W0, lvl_count, entry_count, last_pixel=True):
    rng = np.random.default_rng(seed)
    n_img = len(lvl_count)
    keys = ((rng.integers(0, 255, (n_img, lvl_max_kp)).astype(np.uint32) << 24) |
            rng.integers(0, Hl * Wl, (n_img, lvl_max_kp)).astype(np.uint32))
    if last_pixel:
        keys[:, 0] = (np.uint32(7) << 24) | np.uint32(Hl * Wl - 1)
    desc = rng.integers(0, 2 ** 63, (n_img, lvl_max_kp, 4)).astype(np.uint64)
    ang = rng.integers(0, 30, (n_img, lvl_max_kp)).astype(np.uint8)
    return dict(name=name, lvl_max_kp=lvl_max_kp, max_kp=max_kp, Hl=Hl, Wl=Wl, level=level, H0=H0, W0=W0, keys=keys,
                desc=desc, angle=ang, lvl_count=np.asarray(lvl_count, np.int32), entry_count=np.asarray(entry_count, np.int32))


APPEND_FILL = 0x5A
APPEND_CASES = {c["name"]: c for c in (
    # negative level counts (on a list with room, an empty one and a full one); a list that is full on entry and lists
    # whose count is ABOVE max_kp on entry: nothing is appended and the count stays
    _append_case("negative_and_overfull", 1, 48, 45, 100, 133, 1, 120, 160, [-1, -1000, -7, 5, 5, 60, 0, 9, 3],
                 [10, 0, 45, 45, 46, 60, 50, 40, 0]),
    # level counts around the 256-thread stride; level 255; a level LARGER than level 0
    _append_case("stride_level255_larger_level", 2, 1000, 1100, 144, 192, 255, 120, 160, [255, 256, 257, 1000, 1000, 1],
                 [0, 3, 0, 100, 400, 1099]),
    # H0 W0 = 2^24: the last pixel's position is the whole 24-bit field; from a level of the same size and a smaller one
    _append_case("last_pixel_of_2p24_same_size", 3, 4, 6, 4096, 4096, 0, 4096, 4096, [4, 2], [0, 3]),
    _append_case("last_pixel_of_2p24_smaller_level", 4, 4, 6, 3413, 3413, 1, 4096, 4096, [4, 9], [2, 5]),
)}
APPEND_NULLS = ((False, False), (True, False), (False, True), (True, True))      # (kp_level NULL, kp_xy_q4 NULL)


def append_entry(c):
    """The merged lists on entry: every slot holds the fill (keys: VUS_KEY_INVALID), kp_count the case's entry counts."""
    m = track_ref.new_merged(len(c["lvl_count"]), c["max_kp"], APPEND_FILL)
    m["kp_count"][:] = c["entry_count"]
    return m


@functools.lru_cache(maxsize=None)
def append_reference(name):
    c = APPEND_CASES[name]
    m = track_ref.pyramid_append(c["keys"], c["lvl_count"], c["desc"], c["angle"], c["Hl"], c["Wl"], c["level"], c["H0"], c["W0"],
                                 append_entry(c))
    for v in m.values():
        v.setflags(write=False)
    return m
