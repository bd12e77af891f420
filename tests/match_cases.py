"""The inputs of tests/test_match_contract_gpu.py, built by one function, case(name), which tests/test_match_ref.py uses as
well: there the reference's two old-behaviour switches (match_ref.py) must change the result of every call aimed at
them, which is the proof that these inputs tell a kernel that ignores the contract of include/vus.h from one that holds
it.  Nothing here calls a kernel or the oracle.

A Case is one descriptor / key buffer and a tuple of Calls on it; a Call is one vus_hamming_match with its own counts,
image size, index tables and gate = (max_dy, min_disp, max_disp, max_dist).  Call.aim names the old behaviour the call
would expose: "counts" (a train count above max_kp read as it is), "rows" (an out-of-image train keypoint moved onto the
last row), "" for none."""
import functools
from typing import NamedTuple

import numpy as np

import match_ref

INT_MAX, INT_MIN = 2**31 - 1, -2**31
KEY_INVALID = np.uint32(match_ref.KEY_INVALID)
MT = 512                       # train tile of hamming_match_kernel (csrc/match.hip)


class Call(NamedTuple):
    label: str
    kp_count: np.ndarray
    H: int
    W: int
    q: np.ndarray
    t: np.ndarray
    gate: tuple
    aim: str


class Case(NamedTuple):
    name: str
    desc: np.ndarray           # uint64 [n_img, max_kp, 4]
    keys: np.ndarray           # uint32 [n_img, max_kp]
    calls: tuple
    notes: dict                # slots the GPU test asserts on by name


def _call(label, kc, H, W, q, t, gate, aim=""):
    return Call(label, np.asarray(kc, np.int64).astype(np.int32), H, W, np.asarray(q, np.int32), np.asarray(t, np.int32),
                tuple(gate), aim)


def random_desc(rng, *shape):
    return rng.integers(0, 2**63, size=shape + (4,), dtype=np.int64).view(np.uint64) ^ \
        (rng.integers(0, 2, size=shape + (4,), dtype=np.uint64) << np.uint64(63))


def flip(d, bits):
    d = d.copy()
    for b in bits:
        d[int(b) // 64] ^= np.uint64(1) << np.uint64(int(b) % 64)
    return d


def _key(rng, pos):
    return (np.uint32(rng.integers(0, 255)) << np.uint32(24)) | np.uint32(pos)


# ---------------------------------------------------------------------------------------------------------------------
COUNT_K = (128, 300)


def counts_of(K):
    return [INT_MIN, -5, 0, 1, K - 1, K, K + 1, K + 1000, INT_MAX]


def _counts_case(K):
    """Ungated, max_kp <= 65535: the matrix-core kernel.  Image 0 is the full list Q.  For every count c there is an image
    X (1 + 2k) that carries c, followed by an image Y (2 + 2k) of exact copies of Q's descriptors: a reader that takes a
    train count above K as it is walks from X into Y and prefers a copy at distance 0 and an index >= K.  X itself holds
    Q's descriptors with 1..40 bits flipped, so the contract's result never has distance 0 with X as the train set.
    Every key is VUS_KEY_INVALID: without a gate positions are not read."""
    rng = np.random.default_rng(7000 + K)
    counts = counts_of(K)
    n_img = 1 + 2 * len(counts)
    desc = np.empty((n_img, K, 4), np.uint64)
    desc[0] = random_desc(rng, K)
    kc = [K]
    for k, c in enumerate(counts):
        perm = rng.permutation(K)
        for j in range(K):
            desc[1 + 2 * k, j] = flip(desc[0, perm[j]], rng.permutation(256)[:1 + j % 40])
        desc[2 + 2 * k] = desc[0, rng.permutation(K)]
        kc += [c, K]
    x = 1 + 2 * np.arange(len(counts))
    q = np.concatenate([np.zeros_like(x), x])
    t = np.concatenate([x, np.zeros_like(x)])
    keys = np.full((n_img, K), KEY_INVALID, np.uint32)
    calls = tuple(_call(f"max_dist={md}", kc, 64, 64, q, t, (-1, 0, 0, md), "counts") for md in (256, 20))
    return Case(f"counts-{K}", desc, keys, calls, {})


# ---------------------------------------------------------------------------------------------------------------------
SCAN_K = (65536, 65541)
SCAN_TRAIN_COUNTS = (1, MT - 1, MT, MT + 1, 2 * MT + 1)
SCAN_NQ = 701


def _scan_case(K):
    """Ungated, max_kp > 65535: the tiled scan without a gate.  Three images (about 6 MB): 0 the queries, 1 a list whose
    count is above max_kp, 2 the trains, whose count changes from call to call around the 512-train tile.  Train slot c
    is copied into a query for every count c used, so a reader that goes one slot past the count finds distance 0; the
    slots far past the counts hold copies of the other image's live descriptors."""
    rng = np.random.default_rng(9000 + K)
    nq, nlive = SCAN_NQ, 2 * MT + 76
    desc = np.empty((3, K, 4), np.uint64)
    Q, O, T = desc[0], desc[1], desc[2]
    T[:nlive] = random_desc(rng, nlive)
    Q[:nq] = random_desc(rng, nq)
    O[:] = random_desc(rng, K)
    T[MT] = T[MT - 1]                                          # an exact tie across the tile boundary
    b = random_desc(rng, 3)
    T[300], T[900] = flip(b[0], [1, 200]), flip(b[0], [2, 100])       # equal distances in different tiles
    T[2 * MT - 1], T[2 * MT] = flip(b[1], [9]), flip(b[1], [5])
    T[100], T[700] = flip(b[2], [1, 2, 3, 4]), flip(b[2], [1, 2, 3])  # the higher index is strictly better
    Q[20], Q[21], Q[22] = b[0], b[1], b[2]
    Q[3] = T[0]                                                # distance 0 to the only train of the count-1 call
    Q[4] = ~T[0]                                               # distance 256 to it
    for k, c in enumerate(SCAN_TRAIN_COUNTS):
        Q[10 + k] = T[c]
    for j in range(60):                                        # distances around max_dist = 40
        Q[30 + j] = flip(T[20 + 7 * j], rng.permutation(256)[:[0, 39, 40, 41, 60, 1][j % 6]])
    T[nlive:] = Q[np.arange(K - nlive) % nq]                   # dead slots: copies of the queries
    Q[nq:] = T[np.arange(K - nq) % nlive]
    O[K - 1] = Q[5]                                            # a match at the highest train index there is
    O[0] = flip(Q[6], [17, 130])
    keys = np.full((3, K), KEY_INVALID, np.uint32)
    calls = [_call(f"trains={c} max_dist={md}", [nq, K + 7, c], 64, 64, [0, 2], [2, 0], (-1, 0, 0, md))
             for c in SCAN_TRAIN_COUNTS for md in (256, 40)]
    calls.append(_call("count above max_kp", [65, K + 7, 1], 64, 64, [0, 1], [1, 2], (-1, 0, 0, 256)))
    return Case(f"scan-{K}", desc, keys, tuple(calls), {})


# ---------------------------------------------------------------------------------------------------------------------
GATED_K, GATED_W = 300, 64
GATED_H = {"rows": 64, "gather": 11000, "scan": 12288}         # the kernel each H selects at max_kp = 300
GATED_GATES = ((5, -64, 64, 256), (0, 0, 20, 256), (63, -64, 64, 40), (INT_MAX, -64, 64, 256))
OUTSIDE = 12288 * GATED_W                                      # a position at or beyond H * W for every H above


def _gated_case():
    """One pair of lists for the three gated kernels.  Valid keypoints lie on rows 0..63.  Train slots 30..34 of image 1
    lie outside the image at every H and carry the exact descriptors of queries on rows 58..63 of image 0, at x inside
    those queries' disparity windows; query slots 20..22 of image 0 lie outside too and carry the descriptors of valid
    trains.  The last gate is wider than any image: with it the out-of-image keypoints are within max_dy of every row
    at every H, whichever row they are given."""
    rng = np.random.default_rng(4242)
    K, W = GATED_K, GATED_W
    desc = random_desc(rng, 2, K)
    keys = np.empty((2, K), np.uint32)
    for n in range(2):
        for j in range(K):
            keys[n, j] = _key(rng, rng.integers(0, 58 * W))
    invalid_score = (np.uint32(0x12) << np.uint32(24)) | np.uint32(match_ref.POS_MASK)

    def put(n, slot, pos, like=None):          # pos: a position, which gets a random score byte, or a whole key
        keys[n, slot] = pos if int(pos) > match_ref.POS_MASK else _key(rng, pos)
        if like is not None:
            desc[n, slot] = desc[like]

    # image 0: queries on the bottom rows, slot -> (row, x)
    bottom = {10: (63, 63), 11: (63, 10), 12: (63, 20), 13: (62, 30), 14: (60, 40), 15: (58, 50), 16: (63, 5), 17: (61, 15),
              18: (59, 25), 19: (63, 63)}
    for slot, (y, x) in bottom.items():
        put(0, slot, y * W + x)
    # image 1: valid trains on the bottom rows, whose descriptors the out-of-image queries of image 0 carry
    for slot, (y, x) in {50: (63, 40), 51: (63, 63), 52: (61, 30)}.items():
        put(1, slot, y * W + x)
    put(0, 20, OUTSIDE, like=(1, 50))
    put(0, 21, KEY_INVALID, like=(1, 51))
    put(0, 22, OUTSIDE + 17, like=(1, 52))
    # image 1: out-of-image trains with the descriptors of bottom-row queries; x = 0, 63, 12, 25, 63
    put(1, 30, OUTSIDE, like=(0, 11))
    put(1, 31, KEY_INVALID, like=(0, 10))
    put(1, 32, OUTSIDE + 12, like=(0, 12))
    put(1, 33, OUTSIDE + 25, like=(0, 13))
    put(1, 34, invalid_score, like=(0, 15))
    put(1, 35, 64 * W - 1, like=(0, 19))                       # valid: the last pixel of the smallest image
    # image 1 has 297 live slots; the dead ones are valid copies a reader past the count would take
    put(1, 297, 63 * W + 5, like=(0, 11))
    put(1, 298, 63 * W + 15, like=(0, 12))
    put(1, 299, 63 * W + 60, like=(0, 10))
    kc = [K, K - 3]
    calls = []
    for path, H in GATED_H.items():
        for g, gate in enumerate(GATED_GATES):
            aimed = path == "rows" or gate[0] == INT_MAX
            calls.append(_call(f"{path} gate{g}", kc, H, W, [0, 1, 0], [1, 0, 0], gate, "rows" if aimed else ""))
    calls.append(_call("ungated", kc, 64, W, [0, 1, 0], [1, 0, 0], (-1, 0, 0, 256)))
    notes = {"outside_queries": {20: 50, 21: 51, 22: 52},      # image 0 slot -> its descriptor's train slot in image 1
             "outside_trains": {11: 30, 10: 31, 12: 32, 13: 33, 15: 34},   # image 0 query slot -> out-of-image train
             "last_pixel": (19, 35)}
    return Case("gated", desc, keys, tuple(calls), notes)


# ---------------------------------------------------------------------------------------------------------------------
WORKLOAD = {"rows": (2000, 720, 640), "gather": (2049, 720, 640)}


def _workload_case(path):
    """VUS_KEY_INVALID inside the counted part of both lists, as vus_select_topk leaves it in an overflowed list, at the
    sizes the workload's dispatch sends to the LDS-resident kernel and to the gathering one.  The invalid slots carry the
    descriptors of the other image's keypoints on the bottom rows, at x inside the stereo window behind x = 255, the x
    that 0xFFFFFF has at W = 640."""
    K, H, W = WORKLOAD[path]
    rng = np.random.default_rng(K)
    desc = random_desc(rng, 2, K)
    pos = rng.integers(0, H * W, (2, K))
    keys = ((rng.integers(0, 255, (2, K)).astype(np.uint32) << np.uint32(24)) | pos.astype(np.uint32))
    x_inv = match_ref.POS_MASK % W
    n_inv = 12
    for n in range(2):
        for i in range(n_inv):
            slot = 100 + i
            # as a query left of the invalid train (dx = 10 i), and as one right of it (dx = -10 i) for the other direction
            x = x_inv + 10 * i if n == 0 else x_inv - 10 * i
            keys[n, slot] = _key(rng, (H - 1 - i % 6) * W + x)
    for n in range(2):
        for i in range(n_inv):
            keys[n, K - n_inv + i] = KEY_INVALID
            desc[n, K - n_inv + i] = desc[1 - n, 100 + i]
    calls = (_call("stereo", [K, K], H, W, [0, 1], [1, 0], (5, 0, 128, 64), "rows"),
             _call("stereo reversed window", [K, K], H, W, [0, 1], [1, 0], (5, -128, 0, 256), "rows"))
    return Case(f"workload-{path}", desc, keys, calls, {"n_inv": n_inv})


# ---------------------------------------------------------------------------------------------------------------------
def _tables_case():
    """Index tables: self pairs and a pair listed three times, with a gate and without."""
    rng = np.random.default_rng(55)
    K, H, W = 130, 48, 64
    desc = random_desc(rng, 3, K)
    desc[1, :60] = desc[0, 60:120]
    keys = np.empty((3, K), np.uint32)
    for n in range(3):
        for j in range(K):
            keys[n, j] = _key(rng, rng.integers(0, H * W))
    q, t = [0, 1, 2, 0, 1, 0, 2], [0, 1, 2, 1, 0, 1, 0]
    kc = [K, K - 1, 77]
    calls = (_call("gated", kc, H, W, q, t, (4, -30, 30, 256)), _call("ungated", kc, H, W, q, t, (-1, 0, 0, 256)))
    return Case("tables", desc, keys, calls, {"same": (3, 5), "self": (0, 1, 2)})


def _many_pairs_case():
    """65535 pairs, the most the entry point takes, of one-slot lists."""
    rng = np.random.default_rng(56)
    n_img, H, W = 7, 16, 16
    desc = random_desc(rng, n_img, 1)
    desc[3] = desc[1]
    desc[5] = flip(desc[2, 0], range(40))[None]
    keys = np.array([[_key(rng, p)] for p in (0, 17, 255, 18, 256, 16, int(KEY_INVALID) & match_ref.POS_MASK)], np.uint32)
    kc = [1, 1, 1, 2, 0, 1, 1]
    q, t = rng.integers(0, n_img, 65535), rng.integers(0, n_img, 65535)
    q[:49], t[:49] = np.repeat(np.arange(7), 7), np.tile(np.arange(7), 7)      # every pair of images at least once
    calls = (_call("gated", kc, H, W, q, t, (1, -2, 2, 256)), _call("ungated", kc, H, W, q, t, (-1, 0, 0, 39)))
    return Case("many-pairs", desc, keys, calls, {})


_BUILDERS = {**{f"counts-{K}": functools.partial(_counts_case, K) for K in COUNT_K},
             **{f"scan-{K}": functools.partial(_scan_case, K) for K in SCAN_K},
             "gated": _gated_case,
             **{f"workload-{p}": functools.partial(_workload_case, p) for p in WORKLOAD},
             "tables": _tables_case, "many-pairs": _many_pairs_case}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    for a in (c.desc, c.keys) + tuple(x for call in c.calls for x in (call.kp_count, call.q, call.t)):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, i, **switches):
    """match_ref's result for call i of a case, computed once.  A pair's rows depend on its two images alone, so the
    reference runs once per distinct pair and the rows are copied to wherever the tables list it."""
    c = case(name)
    call = c.calls[i]
    pairs, inverse = np.unique(np.stack([call.q, call.t], axis=1), axis=0, return_inverse=True)
    idx, dist = match_ref.hamming_match(c.desc, c.keys, call.kp_count, call.H, call.W, pairs[:, 0], pairs[:, 1], *call.gate,
                                        **switches)
    idx, dist = idx[inverse.reshape(-1)], dist[inverse.reshape(-1)]
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist
