"""GPU parity of vus_select_topk and of the row-gated vus_hamming_match against the C oracle, bit for bit, at the
edges of their contracts: list lengths around max_kp and cand_cap, sort sizes around the workgroup shapes, boundary
buckets from one key to the whole list, and every host-side dispatch boundary of the stereo matcher."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID = np.uint32(0xFFFFFFFF)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_select(keys, cnt, max_kp):
    import visual_underwater_slam_amd._lib as L
    n, cap = keys.shape
    kp = torch.full((n, max_kp), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    kc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_keys, d_cnt = _dev(keys.view(np.int32)), _dev(cnt.astype(np.int32))
    L.call("vus_select_topk", d_keys.data_ptr(), d_cnt.data_ptr(), n, cap, max_kp, kp.data_ptr(), kc.data_ptr(),
           L.current_stream_ptr())
    torch.cuda.synchronize()
    return kp.cpu().numpy().view(np.uint32), kc.cpu().numpy()


def _check_select(oracle, keys, cnt, max_kp):
    keys = np.ascontiguousarray(keys, np.uint32)
    cnt = np.asarray(cnt, np.int32)
    kp, kc = _gpu_select(keys, cnt, max_kp)
    ekp, ekc = oracle.select_topk(keys, cnt, max_kp)
    assert np.array_equal(kc, ekc)
    bad = np.nonzero((kp != ekp).any(axis=1))[0]
    assert bad.size == 0, f"images {bad[:8]} differ (counts {cnt[bad[:8]]}, max_kp {max_kp})"
    return ekp, ekc


def _unique_keys(rng, n, cap, score_lo=0, score_hi=256):
    """n lists of cap unique keys: random score byte in [score_lo, score_hi), unique positions."""
    out = np.empty((n, cap), np.uint32)
    for i in range(n):
        pos = rng.permutation(1 << 20)[:cap].astype(np.uint32)
        out[i] = (rng.integers(score_lo, score_hi, cap).astype(np.uint32) << 24) | pos
    return out


@pytest.mark.parametrize("order", ["random", "ascending", "descending"])
@pytest.mark.parametrize("max_kp", [1, 63, 64, 65, 2000, 2048, 8192])
def test_select_counts_around_max_kp_and_cand_cap(gpu, oracle, max_kp, order):
    """cand_count of 0, 1, max_kp - 1, max_kp, max_kp + 1, just under cand_cap and above it (clamped), as seven images of
    one launch."""
    rng = np.random.default_rng(100 + max_kp)
    cap = max(2 * max_kp + 100, 5000)
    cnt = np.array([0, 1, max_kp - 1, max_kp, max_kp + 1, cap - 1, cap + 5], np.int32)
    keys = _unique_keys(rng, len(cnt), cap, 40, 200)
    if order != "random":
        for i, c in enumerate(np.minimum(cnt, cap)):
            s = np.sort(keys[i, :c])
            keys[i, :c] = s if order == "ascending" else s[::-1]
    ekp, ekc = _check_select(oracle, keys, cnt, max_kp)
    assert np.array_equal(ekc, np.minimum(max_kp, np.minimum(cnt, cap)))
    assert (ekp[0] == INVALID).all()


@pytest.mark.parametrize("max_kp", [1, 64, 500, 2000, 8192])
@pytest.mark.parametrize("cnt", [300, 3500, 30000])
def test_select_single_score_boundary_bucket_is_the_whole_list(gpu, oracle, max_kp, cnt):
    rng = np.random.default_rng(7)
    keys = _unique_keys(rng, 2, 30000, 178, 179)
    _check_select(oracle, keys, [cnt, cnt - 1], max_kp)


@pytest.mark.parametrize("second", [5, 200, 256, 257, 3000])
def test_select_two_scores_cut_inside_the_second(gpu, oracle, second):
    """1900 keys of the better score, `second` of the next one, max_kp 2000: the boundary bucket holds `second` keys,
    on each side of the length up to which it is ranked in LDS."""
    rng = np.random.default_rng(second)
    cap = 6000
    pos = rng.permutation(1 << 20)[:1900 + second].astype(np.uint32)
    k = np.concatenate([(np.uint32(60) << 24) | pos[:1900], (np.uint32(61) << 24) | pos[1900:]])
    keys = np.full((3, cap), INVALID, np.uint32)
    for i in range(3):
        keys[i, :k.size] = rng.permutation(k)
    cnt = [k.size, k.size, max(k.size - 50, 1901)]
    for max_kp in (2000, 1901, 1900 + second):
        _check_select(oracle, keys, cnt, max_kp)


@pytest.mark.parametrize("n_valid,cnt,max_kp", [(1500, 3000, 2000), (1995, 2005, 2000), (1999, 2300, 2000), (0, 900, 64),
                                                (2100, 2400, 2000), (10, 40, 2000), (3, 9000, 8192)])
def test_select_list_with_invalid_entries_in_its_counted_part(gpu, oracle, n_valid, cnt, max_kp):
    """The overflow tail of the merge kernel: VUS_KEY_INVALID entries inside the counted part sort last like any key."""
    rng = np.random.default_rng(n_valid)
    cap = 9000
    keys = np.full((2, cap), INVALID, np.uint32)
    keys[0, :n_valid] = _unique_keys(rng, 1, n_valid, 30, 256)[0] if n_valid else 0
    keys[1, :cnt] = rng.permutation(keys[0, :cnt])       # the invalid entries anywhere in the list
    ekp, ekc = _check_select(oracle, keys, [cnt, cnt], max_kp)
    assert (ekc == min(cnt, max_kp)).all()
    assert ((ekp[0] != INVALID).sum() == min(n_valid, max_kp))


@pytest.mark.parametrize("max_kp", [2000, 8192])
def test_select_cand_cap_100000_full_list(gpu, oracle, max_kp):
    """Lists far longer than a workgroup keeps in registers (16 per lane): the streamed tail of both passes."""
    rng = np.random.default_rng(3)
    cap = 100000
    keys = np.stack([(rng.integers(0, 256, cap).astype(np.uint32) << 24) | rng.permutation(1 << 22)[:cap].astype(np.uint32)
                     for _ in range(3)])
    keys[2] = (np.uint32(99) << 24) | (keys[2] & np.uint32(0xFFFFFF))        # one score: the radix fallback on a long list
    _check_select(oracle, keys, [cap, cap + 1000, cap], max_kp)


@pytest.mark.parametrize("max_kp", [40, 700, 2000])
def test_select_many_images_with_different_counts(gpu, oracle, max_kp):
    rng = np.random.default_rng(max_kp)
    n, cap = 400, 6000
    keys = _unique_keys(rng, n, cap, 100, 140)       # 40 occupied score bins: boundary buckets of ~ cnt / 40 keys
    cnt = rng.integers(0, cap + 200, n).astype(np.int32)
    cnt[::7] = rng.integers(max(max_kp - 3, 0), max_kp + 4, cnt[::7].size)
    _check_select(oracle, keys, cnt, max_kp)


# ---------------------------------------------------------------------------------------------------------------------
def _stereo_set(rng, n_img, K, H, W, one_row=None):
    desc = rng.integers(0, 2**63, size=(n_img, K, 4), dtype=np.int64).view(np.uint64)
    desc ^= rng.integers(0, 2, size=desc.shape, dtype=np.uint64) << np.uint64(63)
    y = rng.integers(0, H, (n_img, K)) if one_row is None else np.full((n_img, K), one_row)
    x = rng.integers(0, W, (n_img, K))
    kp = ((rng.integers(0, 256, (n_img, K)).astype(np.uint32) << 24) | (y * W + x).astype(np.uint32))
    return desc, kp


def _gpu_match(desc, kp, kc, H, W, q, t, gate):
    import visual_underwater_slam_amd._lib as L
    K = kp.shape[1]
    q, t = np.asarray(q, np.int32), np.asarray(t, np.int32)
    idx = torch.full((len(q), K), -99, dtype=torch.int32, device="cuda")
    dist = torch.full((len(q), K), -99, dtype=torch.int32, device="cuda")
    d_desc, d_kp, d_kc = _dev(desc.view(np.int64)), _dev(kp.view(np.int32)), _dev(np.asarray(kc, np.int32))
    d_q, d_t = _dev(q), _dev(t)
    L.call("vus_hamming_match", d_desc.data_ptr(), d_kp.data_ptr(), d_kc.data_ptr(), K, H, W, d_q.data_ptr(),
           d_t.data_ptr(), len(q), *gate, idx.data_ptr(), dist.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check_match(oracle, desc, kp, kc, H, W, q, t, gate):
    """gate = (max_dy, min_disp, max_disp, max_dist).  Library and oracle both clamp the counts to max_kp (include/vus.h),
    so the oracle takes them as they are."""
    idx, dist = _gpu_match(desc, kp, kc, H, W, q, t, gate)
    eidx, edist = oracle.hamming_match(desc, kp, np.asarray(kc, np.int32), W, q, t, *gate, H=H)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(dist, edist)
    return eidx, edist


# (max_kp, H) on each side of every reachable dispatch boundary of vus_hamming_match: the LDS-resident kernel serves
# max_kp <= 2048 with 36 max_kp + 4 (2 H + 1) <= 96 KiB, the gathering kernel 4 (2 H + 1 + 2 max_kp) <= 96 KiB, the tiled
# scan the rest.  (The dispatch's H <= 16384 condition cannot decide anything: 8 H alone passes 96 KiB at H = 12288.)
DISPATCH = [(2000, 720), (2048, 720), (2049, 720), (2048, 3071), (2048, 3072), (64, 11999), (64, 12000), (64, 12223),
            (64, 12224), (2049, 10238), (2049, 10239), (1, 1), (65, 33)]


@pytest.mark.parametrize("K,H", DISPATCH)
def test_stereo_every_dispatch_path(gpu, oracle, K, H):
    rng = np.random.default_rng(K * 31 + H)
    W = 640 if H <= 4096 else 64
    desc, kp = _stereo_set(rng, 4, K, H, W)
    if K >= 64:
        desc[1, 40] = desc[1, 3]           # duplicates in a train set, on the same row and inside the window
        kp[1, 40] = kp[1, 3]
        desc[0, 5] = desc[1, 3]
        kp[0, 5] = kp[1, 3]
    kc = [K, K, max(K - 1, 0), K + 9]       # the last one above max_kp: clamped
    q = [0, 1, 2, 3, 0, 3]
    t = [1, 0, 3, 2, 0, 3]
    eidx, edist = _check_match(oracle, desc, kp, kc, H, W, q, t, (5, -20, 128, 256))
    if K >= 64:
        assert eidx[0, 5] == 3 and edist[0, 5] == 0      # the lower train index of the two identical descriptors
    _check_match(oracle, desc, kp, kc, H, W, q, t, (2, 0, 60, 90))


@pytest.mark.parametrize("K", [1, 500, 2000, 2100])
def test_stereo_counts_0_1_max_kp_and_above(gpu, oracle, K):
    rng = np.random.default_rng(K)
    H, W = 480, 640
    desc, kp = _stereo_set(rng, 5, K, H, W)
    kc = [0, 1, K, K + 1000, K // 2]
    q = [0, 1, 2, 3, 4, 2, 0, 3, 1, 2]
    t = [2, 2, 0, 2, 3, 1, 0, 3, 1, 4]
    eidx, edist = _check_match(oracle, desc, kp, kc, H, W, q, t, (8, -640, 640, 256))
    assert (eidx[0] == -1).all() and (edist[2] == 512).all()      # empty query set; empty train set


@pytest.mark.parametrize("K", [700, 2000, 2100])
@pytest.mark.parametrize("row", [0, 359, 719])
def test_stereo_all_train_keypoints_on_one_row_and_gate_outside_the_image(gpu, oracle, K, row):
    """One bucket holds the whole train set; rows 0 and H - 1 with a gate that reaches outside the image."""
    rng = np.random.default_rng(K + row)
    H, W = 720, 640
    desc, kp = _stereo_set(rng, 2, K, H, W, one_row=row)
    y = rng.choice([0, 1, 5, 6, 353, 359, 365, 713, 714, 718, 719], K)
    kp[0] = (kp[0] & np.uint32(0xFF000000)) | (y * W + rng.integers(0, W, K)).astype(np.uint32)
    desc[1, 77] = desc[1, 12]
    desc[1, 400] = desc[1, 12]
    desc[0, 9] = desc[1, 12]
    kp[0, 9] = (kp[0, 9] & np.uint32(0xFF000000)) | np.uint32(row * W + 639)
    eidx, _ = _check_match(oracle, desc, kp, [K, K], H, W, [0, 1], [1, 0], (6, -640, 640, 256))
    assert eidx[0, 9] == 12
    _check_match(oracle, desc, kp, [K, K], H, W, [0, 1], [1, 0], (720, 0, 100, 64))


@pytest.mark.parametrize("K", [900, 2100])
def test_stereo_max_dy_0_and_a_window_that_excludes_everything(gpu, oracle, K):
    rng = np.random.default_rng(K)
    H, W = 100, 640
    desc, kp = _stereo_set(rng, 2, K, H, W)
    _check_match(oracle, desc, kp, [K, K - 3], H, W, [0, 1], [1, 0], (0, -640, 640, 256))
    eidx, edist = _check_match(oracle, desc, kp, [K, K - 3], H, W, [0, 1], [1, 0], (5, 700, 900, 256))
    assert (eidx == -1).all() and (edist == 512).all()
    eidx, _ = _check_match(oracle, desc, kp, [K, K - 3], H, W, [0, 1], [1, 0], (5, 0, 128, 0))   # max_dist 0: none accepted
    assert (eidx == -1).all()


def test_stereo_1000_pairs_at_the_headline_size(gpu, oracle):
    """The launch shape of the headline workload (1000 pairs, 2000 keypoints, 1280 x 720), checked at both ends and in the
    middle."""
    rng = np.random.default_rng(5)
    n_pairs, K, H, W = 1000, 2000, 720, 1280
    desc, kp = _stereo_set(rng, 2 * n_pairs, K, H, W)
    kc = rng.integers(1900, 2001, 2 * n_pairs).astype(np.int32)
    q = 2 * np.arange(n_pairs, dtype=np.int32)
    gate = (5, 0, 128, 256)
    idx, dist = _gpu_match(desc, kp, kc, H, W, q, q + 1, gate)
    sel = np.array([0, 1, 2, 498, 499, 500, 501, 997, 998, 999])
    eidx, edist = oracle.hamming_match(desc, kp, kc, W, q[sel], q[sel] + 1, *gate, H=H)
    assert np.array_equal(idx[sel], eidx)
    assert np.array_equal(dist[sel], edist)
    assert (eidx >= 0).sum() > 1000          # the gate leaves real work
