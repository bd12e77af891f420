"""match_ref.py, the numpy statement of the vus_hamming_match contract, against the C oracle on inputs inside the
contract, and the proof that the inputs of tests/test_match_contract_gpu.py (match_cases.py) discriminate: on every call
aimed at one of the two behaviours single kernels had before the contract was written down, switching that behaviour on
in the reference changes output slots.  No GPU."""
import numpy as np
import pytest

import match_cases as C
import match_ref as R


def _set(rng, n_img, K, H, W):
    desc = C.random_desc(rng, n_img, K)
    pos = rng.integers(0, H * W, (n_img, K)).astype(np.uint32)
    keys = (rng.integers(0, 256, (n_img, K)).astype(np.uint32) << np.uint32(24)) | pos
    return desc, keys


GATES = [(-1, 0, 0, 256), (-1, 0, 0, 100), (5, -20, 40, 256), (0, 0, 64, 256), (3, 1, 9, 110), (48, -64, 64, 0),
         (2**31 - 1, -5, 5, 256)]


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("K", [1, 37, 260])
def test_reference_equals_the_oracle_inside_the_contract(oracle, K, gate):
    """Counts in [0, max_kp] (empty lists among them), positions inside the image, duplicates of descriptors and of whole
    keypoints: both implementations of the contract agree bit for bit."""
    rng = np.random.default_rng(K * 100 + gate[0] % 97)
    H, W = 48, 64
    desc, keys = _set(rng, 5, K, H, W)
    if K > 30:
        desc[1, 20] = desc[1, 3]                        # duplicates in a train set: same keypoint, then same descriptor
        keys[1, 20] = keys[1, 3]
        desc[1, 25] = desc[1, 3]
        desc[0, 5], keys[0, 5] = desc[1, 3], keys[1, 3]
        desc[2, :30] = desc[0, :30]
    kc = np.array([K, K, max(K - 1, 0), 0, (K + 1) // 2], np.int32)
    q = [0, 1, 2, 3, 4, 0, 0, 2, 4]
    t = [1, 0, 4, 0, 3, 0, 2, 2, 1]
    idx, dist = R.hamming_match(desc, keys, kc, H, W, q, t, *gate)
    eidx, edist = oracle.hamming_match(desc, keys, kc, W, q, t, *gate, H=H)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(dist, edist)
    assert (idx[3] == -1).all() and (dist[4] == R.NO_CANDIDATE).all()      # empty query list; empty train list
    if K > 30 and gate[3] > 0 and (gate[0] < 0 or gate[1] <= 0 <= gate[2]):
        assert idx[0, 5] == 3 and dist[0, 5] == 0       # the lowest of the three equal trains


def test_reference_equals_the_oracle_outside_the_image_and_above_max_kp(oracle):
    """The oracle holds the same two rules: counts clamped to [0, max_kp], and under a gate no part for a keypoint at or
    beyond H * W."""
    rng = np.random.default_rng(3)
    K, H, W = 90, 48, 64
    desc, keys = _set(rng, 4, K, H, W)
    keys[0, 10:14] = [H * W, 0xFFFFFFFF, H * W + 7, H * W - 1]
    keys[1, 30:33] = [H * W, 0xFFFFFFFF, H * W + 7]
    desc[1, 30:33] = desc[0, 40:43]
    keys[0, 40:43] = [(H - 1) * W + 20, (H - 1) * W + 63, (H - 2) * W + 9]
    kc = np.array([K + 5, 2**31 - 1, -2**31, -1], np.int32)
    for gate in [(-1, 0, 0, 256), (4, -64, 64, 256), (2**31 - 1, -64, 64, 256)]:
        idx, dist = R.hamming_match(desc, keys, kc, H, W, [0, 1, 2, 0, 3], [1, 0, 0, 2, 3], *gate)
        eidx, edist = oracle.hamming_match(desc, keys, kc, W, [0, 1, 2, 0, 3], [1, 0, 0, 2, 3], *gate, H=H)
        assert np.array_equal(idx, eidx)
        assert np.array_equal(dist, edist)
        if gate[0] >= 0:
            assert (idx[0, 10:13] == -1).all() and (dist[0, 10:13] == R.NO_CANDIDATE).all() and idx[0, 13] >= 0
            assert not np.isin(idx[0], [30, 31, 32]).any()
        else:
            assert (idx[0, 40:43] == [30, 31, 32]).all()


def test_reference_chunks_its_queries(monkeypatch):
    rng = np.random.default_rng(4)
    desc, keys = _set(rng, 2, 300, 48, 64)
    whole = R.hamming_match(desc, keys, [300, 299], 48, 64, [0, 1], [1, 0], 6, -30, 30, 120)
    monkeypatch.setattr(R, "_TEMP_BYTES", 7 * 32 * 299)             # seven queries at a time
    parts = R.hamming_match(desc, keys, [300, 299], 48, 64, [0, 1], [1, 0], 6, -30, 30, 120)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])


def test_popcount_table_equals_the_bit_loop(monkeypatch):
    rng = np.random.default_rng(5)
    x = C.random_desc(rng, 50)
    x[0], x[1] = 0, ~np.uint64(0)
    slow = np.array([[bin(int(v)).count("1") for v in row] for row in x])
    assert np.array_equal(R._popcount(x), slow)
    if hasattr(np, "bitwise_count"):
        monkeypatch.delattr(np, "bitwise_count")
        assert np.array_equal(R._popcount(x), slow)


AIMED = [(name, i) for name in C.NAMES if not name.startswith("scan") for i, call in enumerate(C.case(name).calls) if call.aim]


def test_some_calls_are_aimed_at_each_old_behaviour():
    aims = {C.case(name).calls[i].aim for name, i in AIMED}
    assert aims == {"counts", "rows"}
    names = {name for name, _ in AIMED}
    assert {f"counts-{K}" for K in C.COUNT_K} | {"gated"} | {f"workload-{p}" for p in C.WORKLOAD} <= names
    gated = C.case("gated")
    for path in C.GATED_H:          # every gated kernel has a call that would expose it
        assert any(call.aim == "rows" and call.label.startswith(path) for call in gated.calls)


@pytest.mark.parametrize("name,i", AIMED, ids=[f"{n}/{C.case(n).calls[i].label}" for n, i in AIMED])
def test_old_behaviour_changes_slots_of_every_call_aimed_at_it(name, i):
    case, call = C.case(name), C.case(name).calls[i]
    K = case.keys.shape[1]
    switch = {"counts": {"clamp_counts": False}, "rows": {"clamp_rows": True}}[call.aim]
    idx, dist = C.reference(name, i)
    oidx, odist = C.reference(name, i, **switch)
    differ = ((idx != oidx) | (dist != odist)).sum(axis=1)
    print(f"{name} / {call.label}: slots that differ per pair under {switch}: {differ.tolist()}")
    if call.aim == "counts":
        # every pair whose train count is above max_kp, with a query list that is not empty
        hit = (call.kp_count[call.t].astype(np.int64) > K) & (call.kp_count[call.q] > 0)
        assert hit.sum() == 3
        assert (differ[hit] > 0).all()
        assert (differ[~hit] == 0).all()
        assert (oidx[hit] >= K).any(axis=1).all()       # the unclamped reader returns indices past the list
    else:
        # every pair with two different images: each direction has out-of-image trains in front of bottom-row queries
        hit = call.q != call.t
        assert hit.sum() >= 2
        assert (differ[hit] > 0).all()
    # the other switch leaves these calls alone where it cannot apply
    if call.aim == "counts":
        assert all(np.array_equal(a, b) for a, b in zip(C.reference(name, i, clamp_rows=True), (idx, dist)))
