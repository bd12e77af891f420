"""vus_keyframe_similarity (csrc/retrieve.hip: keyframe similarity as an FP4 block-scaled GEMM) against its numpy statement
(tests/retrieval_ref.py), with EXACT equality of S: counts around the 128-row LDS chunk, the 32-row tile, the 512-query
workgroup and the 32-query column tile; `top` below and above the counts; distances at the bound and at the extremes;
dead slots that hold exact copies; every form of t_limit on a poisoned S; image numbers out of range and repeated; the
smallest shapes; and one shape at the workload's width.  The descriptor construction is that of
tests/test_hamming_fp4_gpu.py: images that are permutations of each other with up to 40 flipped bits."""
import numpy as np
import pytest
import torch

import retrieval_ref as R

pytestmark = pytest.mark.gpu

CHUNK, QWG, TRAIN_BLOCK = 128, 512, 8   # KS_CHUNK, KS_QWG and KS_TB of csrc/retrieve.hip
POISON = 0x5A5A5A5A


def _random_desc(rng, n_img, K):
    return rng.integers(0, 2**63, size=(n_img, K, 4), dtype=np.int64).view(np.uint64) ^ \
        (rng.integers(0, 2, size=(n_img, K, 4), dtype=np.uint64) << np.uint64(63))


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


def _permuted_images(rng, n_img, K):
    """Image i = image i-1 permuted, slot j with j % 41 bit flips (a bit drawn twice flips back)."""
    desc = _random_desc(rng, n_img, K)
    rows = np.arange(K)
    for i in range(1, n_img):
        desc[i] = desc[i - 1, rng.permutation(K)]
        for s in range(40):
            on = rows[(rows % 41) > s]
            bits = rng.integers(0, 256, size=len(on))
            desc[i, on, bits // 64] ^= np.uint64(1) << (bits % 64).astype(np.uint64)
    return desc


def _similarity(desc, kc, q_img, t_img, t_limit, top, max_dist):
    """S of the entry point as a host array; S is poisoned before the call."""
    import visual_underwater_slam_amd._lib as L
    n_img, K, _ = desc.shape
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()
    d, c = dev(desc.view(np.int64), np.int64), dev(kc, np.int32)
    q, t = dev(q_img, np.int32), dev(t_img, np.int32)
    lim = None if t_limit is None else dev(t_limit, np.int32)
    S = torch.full((len(q_img), len(t_img)), POISON, dtype=torch.int32, device="cuda")
    L.call("vus_keyframe_similarity", d.data_ptr(), c.data_ptr(), n_img, K, q.data_ptr(), len(q_img), t.data_ptr(), len(t_img),
           L.ptr(lim), top, max_dist, S.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    return S.cpu().numpy()


def _check(desc, kc, q_img, t_img, t_limit, top, max_dist):
    got = _similarity(desc, kc, q_img, t_img, t_limit, top, max_dist)
    want = R.keyframe_similarity(desc, kc, q_img, t_img, t_limit, top, max_dist)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    return got


K_EDGE = 1100                                   # max_kp not a multiple of 32
COUNTS = [0, -5, 1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 31, QWG - 33, QWG - 1, QWG, QWG + 1, QWG + 32,
          2 * QWG + 1, K_EDGE - 1, K_EDGE, K_EDGE + 7]


@pytest.fixture(scope="module")
def edge_images(gpu):
    rng = np.random.default_rng(41)
    return _permuted_images(rng, len(COUNTS), K_EDGE), np.array(COUNTS, np.int32)


@pytest.mark.parametrize("top", [1, 32, 512, 513, 1100])
def test_counts_and_top_at_the_tile_edges(edge_images, top):
    desc, kc = edge_images
    img = np.arange(len(COUNTS))
    S = _check(desc, kc, img, img, None, top, 35)          # all ordered pairs, the self pairs included
    nq = np.minimum(np.clip(kc, 0, K_EDGE), top)
    assert np.array_equal(np.diag(S), nq)
    assert (S[nq == 0] == 0).all() and (S[:, nq == 0] == 0).all()
    assert (S <= nq[:, None]).all()
    assert top < 512 or ((np.tril(S, -1) > 0).any() and (np.triu(S, 1) > 0).any())      # not the diagonal alone


@pytest.mark.parametrize("max_dist", [0, 35, 256])
def test_neighbours_at_the_bound_in_every_chunk_tile_and_lane_half(gpu, max_dist):
    rng = np.random.default_rng(42 + max_dist)
    K, nt, nq = 640, 600, 590
    desc = _random_desc(rng, 2, K)                          # image 0: queries, image 1: trains; unrelated (~128 bits apart)
    # train slots over the five chunks, the four 32-row tiles of a chunk and both lane halves (rows r with r % 8 >= 4)
    trains = [0, 5, 36, 68, 100, 127, 128, 133, 200, 255, 256, 300, 383, 389, 470, 511, 512, 517, 575, 599]
    queries = [0, 31, 32, 63, 64, 127, 128, 130, 255, 256, 300, 383, 384, 400, 511, 512, 513, 544, 575, 589]
    inside = 0
    for k, (qi, tj) in enumerate(zip(queries, trains)):     # alternately exactly at the bound and one bit past it
        d = min(max_dist + (k & 1), 256)
        desc[0, qi] = _flip(desc[1, tj], rng.permutation(256)[:d])
        inside += d <= max_dist
    kc = np.array([nq, nt], np.int32)
    S = _check(desc, kc, [0, 1], [1, 0], None, K, max_dist)
    assert S[0, 0] == (inside if max_dist < 256 else nq), S
    if max_dist == 256:
        assert S[1, 1] == nt


def test_all_zero_against_all_ones_descriptors(gpu):
    K = 70
    desc = np.zeros((2, K, 4), np.uint64)
    desc[1] = np.uint64(0xFFFFFFFFFFFFFFFF)                 # every dot is -256
    kc = np.array([K, 40], np.int32)
    assert _check(desc, kc, [0, 1], [1, 0], None, K, 255).tolist() == [[0, K], [40, 0]]
    assert _check(desc, kc, [0, 1], [1, 0], None, K, 256).tolist() == [[K, K], [40, 40]]
    assert _check(desc, kc, [0, 1], [0, 1], None, K, 0).tolist() == [[K, 0], [0, 40]]


@pytest.mark.parametrize("max_dist", [0, 35])
def test_dead_slots_hold_exact_copies_and_are_not_seen(gpu, max_dist):
    rng = np.random.default_rng(43)
    K = 700
    desc = _random_desc(rng, 4, K)                          # four unrelated images
    kc = np.array([K, 130, K, 9], np.int32)
    desc[1, 130:] = desc[0, :K - 130]                       # train image 1: every slot at or past its count copies a query of 0
    desc[2, 33:] = desc[0, :K - 33]                         # train image 2 is full: with top = 33 the copies lie past top
    desc[3, 9:] = desc[1, :K - 9]                           # query image 3: its dead slots copy live trains of image 1
    for top in (33, K):
        S = _check(desc, kc, [0, 3, 0, 1], [1, 1, 2, 0], None, top, max_dist)
        assert S[0, 0] == 0 and S[1, 0] == 0, S             # 0 -> 1 and 3 -> 1: nothing but dead slots would match
        assert S[0, 2] == (0 if top == 33 else K - 33), S   # 0 -> 2: the copies count once top lets them in
        assert S[3, 3] == 0 and S[3, 0] == min(130, top), S   # 1 -> 0: no live match; 1 -> 1: itself


def test_t_limit_in_every_form_on_a_poisoned_S(edge_images):
    desc, kc = edge_images
    q_img = [3, 4, 5, 6, 7, 8, 9, 3, 4, 5, 6]               # counts 31 .. 287
    t_img = [9, 8, 7, 6, 5, 4, 3, 9, 8, 7]
    n_t = len(t_img)
    lim = [0, n_t, n_t + 5, -3, 3, 1, TRAIN_BLOCK, TRAIN_BLOCK + 1, TRAIN_BLOCK - 1, 2**31 - 1, -2**31]
    S = _check(desc, kc, q_img, t_img, lim, 512, 35)
    for q, l in enumerate(np.clip(lim, 0, n_t)):
        assert (S[q, l:] == 0).all() and (l == 0 or S[q, :l].any()), (q, S[q])
    full = _check(desc, kc, q_img, t_img, None, 512, 35)
    assert np.array_equal(full[1], S[1]) and np.array_equal(full[2], S[2]) and np.array_equal(full[9], S[9])
    # the triangular pattern of StereoOrbFrontend.keyframe_similarity: t_limit[b] = max(b - min_gap + 1, 0)
    img = np.arange(3, 14)
    square = _check(desc, kc, img, img, None, 512, 35)
    for min_gap in (0, 1, 5, len(img)):
        tri = _check(desc, kc, img, img, np.maximum(np.arange(len(img)) - min_gap + 1, 0), 512, 35)
        assert np.array_equal(tri, np.tril(square, -min_gap))


def test_image_numbers_out_of_range_and_repeated_and_the_smallest_shapes(edge_images):
    desc, kc = edge_images
    n_img = len(COUNTS)
    S = _check(desc, kc, [5, -1, 5, n_img, 10**6, 7, -2**31], [7, 7, n_img, 5, -1, 2**31 - 1, 6, 6], None, 512, 35)
    assert (S[[1, 3, 4, 6]] == 0).all() and (S[:, [2, 4, 5]] == 0).all()
    assert np.array_equal(S[0], S[2]) and np.array_equal(S[:, 0], S[:, 1]) and S[0, 3] == 33 and S[5, 0] == CHUNK
    _check(desc, kc, [16], list(range(n_img)) * 2, None, 1100, 35)          # n_q = 1, five train blocks
    _check(desc, kc, list(range(n_img)), [17], None, 1100, 35)              # n_t = 1
    _check(desc, kc, [12, 13, 14], [15, 16], [2, 1, 2], 513, 35)            # n_q != n_t
    one = np.array([[[1, 2, 3, 4]], [[1, 2, 3, 4]], [[1, 2, 3, 5]], [[9, 9, 9, 9]]], np.uint64)    # max_kp = 1
    for max_dist, want in ((0, [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]), (1, [[1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]])):
        assert _check(one, np.array([1, 1, 1, 0], np.int32), [0, 2, 3], [0, 1, 2, 3], None, 1, max_dist).tolist() == want


def test_two_runs_give_equal_bits(edge_images):
    desc, kc = edge_images
    img = np.arange(len(COUNTS))
    a = _similarity(desc, kc, img, img, None, 1100, 35)
    b = _similarity(desc, kc, img, img, None, 1100, 35)
    assert np.array_equal(a, b) and a.any()


def test_one_shape_at_the_workloads_width(gpu):
    rng = np.random.default_rng(44)
    K, n = 2000, 12
    desc = _permuted_images(rng, n, K)
    kc = np.array([K, K, K, 1999, 1800, K, 400, K, 513, K, K, 2050], np.int32)
    img = np.arange(n)
    S = _check(desc, kc, img, img, np.arange(n) + 1, 512, 35)
    assert np.array_equal(np.diag(S), np.minimum(kc, 512)) and (np.triu(S, 1) == 0).all()
    assert (np.diag(S, -1) > 0).all()
