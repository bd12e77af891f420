"""The ungated track matcher (hamming_match_mfma_kernel: all-pairs Hamming as an FP4 block-scaled GEMM) at the edges of
its tile shape, against the CPU oracle: train counts around the 128-train LDS chunk and the 32-row tile, query counts
around the 512-query workgroup and the 32-query column tile, a max_kp at the 16-bit train-index limit, distances at
the extremes and at max_dist, and exact ties spread over chunks, tiles and lane halves (the lowest index wins)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, QWG = 128, 512   # HM_CHUNK and HM_QWG of csrc/match.hip


def _random_desc(rng, n_img, K):
    return rng.integers(0, 2**63, size=(n_img, K, 4), dtype=np.int64).view(np.uint64) ^ \
        (rng.integers(0, 2, size=(n_img, K, 4), dtype=np.uint64) << np.uint64(63))


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


def _match(desc, kc, q, t, max_dist):
    import visual_underwater_slam_amd._lib as L
    n_img, K, _ = desc.shape
    keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
            for a in (desc.view(np.int64), np.zeros((n_img, K), np.int32), kc.astype(np.int32),
                      np.asarray(q, np.int32), np.asarray(t, np.int32))]
    idx = torch.empty((len(q), K), dtype=torch.int32, device="cuda")
    dist = torch.empty((len(q), K), dtype=torch.int32, device="cuda")
    L.call("vus_hamming_match", keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), K, 64, 64,
           keep[3].data_ptr(), keep[4].data_ptr(), len(q), -1, 0, 0, max_dist, idx.data_ptr(), dist.data_ptr(),
           L.current_stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check(oracle, desc, kc, q, t, max_dist):
    idx, dist = _match(desc, kc, q, t, max_dist)
    eidx, edist = oracle.hamming_match(desc, np.zeros(desc.shape[:2], np.uint32), kc, 64, np.asarray(q, np.int32),
                                       np.asarray(t, np.int32), -1, 0, 0, max_dist, H=64)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(dist, edist)
    return idx, dist


@pytest.mark.parametrize("max_dist", [256, 50])
def test_fp4_matcher_counts_at_chunk_and_column_tile_edges(gpu, oracle, max_dist):
    rng = np.random.default_rng(21)
    K = 1100                                    # max_kp not a multiple of 32
    counts = [1, 31, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 31, 287, QWG - 33, QWG - 1, QWG, QWG + 1, QWG + 32,
              2 * QWG + 1, K - 1, K]
    n = len(counts)
    desc = _random_desc(rng, n, K)
    for i in range(1, n):                       # image i = image i-1 permuted, with up to 40 bit flips per descriptor
        perm = rng.permutation(K)
        for j in range(K):
            desc[i, j] = _flip(desc[i - 1, perm[j]], rng.integers(0, 256, size=j % 41))
    kc = np.array(counts, np.int32)
    q = [i for i in range(n) for j in range(n) if i != j]
    t = [j for i in range(n) for j in range(n) if i != j]
    idx, _ = _check(oracle, desc, kc, q, t, max_dist)
    assert (idx >= 0).any()


def test_fp4_matcher_max_kp_at_the_train_index_limit(gpu, oracle):
    rng = np.random.default_rng(22)
    K = 65535
    desc = np.zeros((3, K, 4), np.uint64)
    desc[:, :3100] = _random_desc(rng, 3, 3100)
    desc[1, :3000] = desc[0, rng.permutation(3000)]
    desc[1, 2999] = desc[0, 2990]               # a tie near the end of the valid trains
    desc[2, :2500] = desc[0, 600:3100]
    kc = np.array([3100, 3000, 2500], np.int32)
    idx, dist = _check(oracle, desc, kc, [0, 1, 2, 0, 1], [1, 0, 0, 2, 2], 256)
    assert (idx[:, 3100:] == -1).all() and (dist[:, 3100:] == 512).all()
    assert (idx[2, :2500] == np.arange(600, 3100)).all() and (dist[2, :2500] == 0).all()


@pytest.mark.parametrize("max_dist", [256, 255, 40])
def test_fp4_matcher_distances_at_the_extremes(gpu, oracle, max_dist):
    rng = np.random.default_rng(23)
    K = 600
    desc = np.zeros((4, K, 4), np.uint64)
    x = _random_desc(rng, 1, 1)[0, 0]
    desc[0, 0] = x                              # image 0: a single train descriptor
    desc[1, 0] = x                              # distance 0
    desc[1, 1] = ~x                             # distance 256: the complement
    desc[1, 2] = np.uint64(0)
    desc[1, 3] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for i, d in enumerate(range(4, 260)):       # every distance 0..255 from the single train
        desc[1, d] = _flip(x, rng.permutation(256)[:i])
    desc[2] = _random_desc(rng, 1, K)[0]        # image 2: random trains; image 3: queries at controlled distances
    for j in range(K):
        desc[3, j] = _flip(desc[2, (7 * j) % K], rng.permutation(256)[:[0, 39, 40, 41, 60, 1][j % 6]])
    kc = np.array([1, 260, K, K], np.int32)
    idx, dist = _check(oracle, desc, kc, [1, 3, 0], [0, 2, 1], max_dist)
    assert dist[0, 0] == 0 and dist[0, 1] == 256 and idx[0, 0] == 0
    assert (dist[0, 4:260] == np.arange(256)).all()
    assert (idx[0, 1] == 0) == (max_dist >= 256)
    if max_dist == 40:
        assert (dist[1, 2:K:6] == 40).all() and (idx[1, 2:K:6] >= 0).all()
        assert (dist[1, 3:K:6] == 41).all() and (idx[1, 3:K:6] == -1).all()


def test_fp4_matcher_ties_go_to_the_lowest_index(gpu, oracle):
    rng = np.random.default_rng(24)
    K = 1200
    desc = _random_desc(rng, 2, K)
    trains, queries = desc[0], desc[1]
    # one descriptor at train indices in lane half 1 of a later chunk, in lane half 0 after it, and in later chunks
    for k, dup in enumerate([[517, 520, 528, 800, 1100], [36, 4, 1199], [255, 256, 511, 512], [1023, 1024, 1056]]):
        v = _random_desc(rng, 1, 1)[0, 0]
        for i in dup:
            trains[i] = v
        for qi in [k, 33 + k, 100 + k, 511 - k, 512 + k, 1000 + k, 1199 - k]:   # spread over column tiles and waves
            queries[qi] = v
    # equal distances to different descriptors: the lower train index wins wherever the two lie
    for k, (lo, hi) in enumerate([(450, 900), (5, 261), (300, 1150), (700, 701), (97, 1119)]):
        base = _random_desc(rng, 1, 1)[0, 0]
        trains[lo] = _flip(base, [3 * k + 1, 200])
        trains[hi] = _flip(base, [3 * k + 2, 100])
        queries[45 + 60 * k] = base               # distance 2 to both
    kc = np.array([K, K], np.int32)
    idx, dist = _check(oracle, desc, kc, [1], [0], 256)
    for k, dup in enumerate([[517, 520, 528, 800, 1100], [36, 4, 1199], [255, 256, 511, 512], [1023, 1024, 1056]]):
        for qi in [k, 33 + k, 100 + k, 511 - k, 512 + k, 1000 + k, 1199 - k]:
            assert idx[0, qi] == min(dup) and dist[0, qi] == 0
    for k, (lo, hi) in enumerate([(450, 900), (5, 261), (300, 1150), (700, 701), (97, 1119)]):
        assert idx[0, 45 + 60 * k] == lo and dist[0, 45 + 60 * k] == 2
