"""Plain numpy statement of the vus_hamming_match contract (include/vus.h), written from the header: one distance matrix
per pair, the gates as boolean masks, argmin for the lowest index among the smallest distances.  It shares no code with
the C oracle or with a kernel.

Two switches reproduce what single kernels did before the contract was written down.  They exist for
tests/test_match_ref.py only, which proves with them that the inputs of tests/test_match_contract_gpu.py tell the old
behaviour from the contract:
  clamp_counts=False  the train count is taken as it is; rows past max_kp are the next images' slots (the buffer is one
                      [n_img * max_kp] array), up to the end of the buffer, and the index returned is the row read
                      (it can be max_kp or more).  The query side is not affected: no kernel ever wrote past max_kp.
  clamp_rows=True     no keypoint is invalid; a train keypoint's row is min(row, H - 1), its x the true one."""
import numpy as np

POS_MASK = 0x00FFFFFF          # VUS_KEY_POS_MASK
KEY_INVALID = 0xFFFFFFFF       # VUS_KEY_INVALID
NO_CANDIDATE = 512
_TEMP_BYTES = 64 << 20         # no temporary of the distance computation is larger than this

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def _popcount(x):
    """Set bits of every uint64 of x."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    return _POP8[x.view(np.uint8).astype(np.intp)].reshape(x.shape + (8,)).sum(axis=-1, dtype=np.uint8)


def _live(count, max_kp):
    return min(max(int(count), 0), max_kp)


def hamming_match(desc, kp_keys, kp_count, H, W, q_index, t_index, max_dy, min_disp, max_disp, max_dist,
                  clamp_counts=True, clamp_rows=False):
    desc = np.ascontiguousarray(desc, np.uint64)
    n_img, K, _ = desc.shape
    flat_desc = desc.reshape(n_img * K, 4)
    flat_pos = (np.ascontiguousarray(kp_keys, np.uint32).reshape(n_img * K) & np.uint32(POS_MASK)).astype(np.int64)
    q_index, t_index = np.asarray(q_index, np.int64).reshape(-1), np.asarray(t_index, np.int64).reshape(-1)
    H, W, max_dy = int(H), int(W), int(max_dy)
    gated = max_dy >= 0
    # the largest temporary per (query, train) cell: the xor, 4 words of 8 bytes; on the table path one index per byte
    per_cell = 32 if hasattr(np, "bitwise_count") else 32 * np.dtype(np.intp).itemsize
    idx = np.full((len(q_index), K), -1, np.int32)
    dist = np.full((len(q_index), K), NO_CANDIDATE, np.int32)
    for p, (qi, ti) in enumerate(zip(q_index, t_index)):
        nq = _live(kp_count[qi], K)
        if clamp_counts:
            nt = _live(kp_count[ti], K)
        else:
            nt = min(max(int(kp_count[ti]), 0), (n_img - ti) * K)
        if nq == 0 or nt == 0:
            continue
        dt = flat_desc[ti * K: ti * K + nt]
        pt = flat_pos[ti * K: ti * K + nt]
        yt, xt = pt // W, pt % W
        if clamp_rows:
            yt = np.minimum(yt, H - 1)
            train_ok = np.ones(nt, bool)
        else:
            train_ok = pt < H * W
        step = max(1, _TEMP_BYTES // (per_cell * nt))
        for i0 in range(0, nq, step):
            i1 = min(nq, i0 + step)
            dq = flat_desc[qi * K + i0: qi * K + i1]
            d = _popcount(dq[:, None, :] ^ dt[None, :, :]).sum(axis=2, dtype=np.int32)        # [queries, trains]
            if gated:
                pq = flat_pos[qi * K + i0: qi * K + i1]
                yq, xq = pq // W, pq % W
                dy, dx = yq[:, None] - yt[None, :], xq[:, None] - xt[None, :]
                ok = (np.abs(dy) <= max_dy) & (dx >= min_disp) & (dx <= max_disp) & train_ok[None, :]
                if not clamp_rows:
                    ok &= (pq < H * W)[:, None]
                d = np.where(ok, d, 1 << 20)
            j = d.argmin(axis=1)                               # the first of equal minima: the lowest train index
            best = d[np.arange(i1 - i0), j]
            found = best < (1 << 20)
            idx[p, i0:i1] = np.where(found & (best <= max_dist), j, -1)
            dist[p, i0:i1] = np.where(found, best, NO_CANDIDATE)
    return idx, dist
