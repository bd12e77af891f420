"""The numpy statement of vus_keyframe_similarity (include/vus_retrieval.h), twice: by popcount of the XOR, and -- independently
-- by the +-1 matrix product the kernel computes (dot = 256 - 2 Hamming).  Test infrastructure only (a plain module, not a
conftest): the CPU tests hold the two forms against each other, the GPU tests hold the kernel to the first."""
import numpy as np

_POP8 = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def _popcount64(x):
    """Set bits of every uint64 of x."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    return _POP8[np.ascontiguousarray(x)[..., None].view(np.uint8)].sum(-1, dtype=np.uint8)


def used_count(kp_count, n_img, max_kp, top, m):
    """Descriptors of image m that take part; 0 for an image number outside [0, n_img)."""
    if m < 0 or m >= n_img:
        return 0
    return min(max(int(kp_count[m]), 0), max_kp, top)


def _limits(t_limit, n_q, n_t):
    if t_limit is None:
        return np.full(n_q, n_t, np.int64)
    return np.clip(np.asarray(t_limit, np.int64), 0, n_t)


def min_hamming(dq, dt):
    """[nq] the smallest Hamming distance of every row of dq [nq, 4] uint64 to the rows of dt [nt, 4] (nt >= 1)."""
    dq, dt = np.ascontiguousarray(dq).view(np.uint64).reshape(-1, 4), np.ascontiguousarray(dt).view(np.uint64).reshape(-1, 4)
    best = np.full(len(dq), 257, np.int64)
    for j0 in range(0, len(dt), 512):                  # [nq, 512] distances at a time, one 64-bit word after the other
        d = np.zeros((len(dq), len(dt[j0:j0 + 512])), np.uint16)
        for w in range(4):
            d += _popcount64(dq[:, None, w] ^ dt[None, j0:j0 + 512, w])
        best = np.minimum(best, d.min(1))
    return best


def max_dot(dq, dt):
    """[nq] the largest dot product of the +-1 forms: bit set -> -1, clear -> +1; float32 like the accumulators."""
    def pm(d):
        bits = np.unpackbits(np.ascontiguousarray(d).view(np.uint8).reshape(len(d), 32), axis=1, bitorder="little")
        return (1.0 - 2.0 * bits).astype(np.float32)
    return (pm(dq) @ pm(dt).T).max(1)


def keyframe_similarity(desc, kp_count, q_img, t_img, t_limit, top, max_dist, form="popcount"):
    """S int32 [n_q, n_t] of the header's SEMANTICS.  desc uint64 [n_img, max_kp, 4]; form "popcount" or "matmul"."""
    desc = np.asarray(desc).view(np.uint64)
    n_img, max_kp, _ = desc.shape
    q_img, t_img = np.asarray(q_img, np.int64).reshape(-1), np.asarray(t_img, np.int64).reshape(-1)
    lim = _limits(t_limit, len(q_img), len(t_img))
    S = np.zeros((len(q_img), len(t_img)), np.int32)
    memo = {}
    for q, qi in enumerate(q_img):
        nq = used_count(kp_count, n_img, max_kp, top, qi)
        for t in range(int(lim[q])):
            ti = t_img[t]
            nt = used_count(kp_count, n_img, max_kp, top, ti)
            if nq == 0 or nt == 0:
                continue
            if (qi, ti) not in memo:
                if form == "popcount":
                    memo[qi, ti] = int((min_hamming(desc[qi, :nq], desc[ti, :nt]) <= max_dist).sum())
                else:
                    memo[qi, ti] = int((max_dot(desc[qi, :nq], desc[ti, :nt]) >= 256 - 2 * max_dist).sum())
            S[q, t] = memo[qi, ti]
    return S
