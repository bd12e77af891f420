"""vus_hamming_match on all five kernels behind it (csrc/match.hip) where include/vus.h states what the suite did not
reach: counts outside [0, max_kp], keypoints at or beyond H * W under a gate and without one, the ungated tiled scan for
max_kp > 65535, and the index tables at their limits.  Every result is compared bit for bit with match_ref.py, the numpy
statement of the contract; that the inputs (match_cases.py) tell the kernels' earlier behaviours from the contract is
shown without a GPU by tests/test_match_ref.py.  Outputs are prefilled with a sentinel: every slot of every pair is
written."""
import numpy as np
import pytest
import torch

import match_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -777


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # a copy: the cases' arrays are read-only


class _Device:
    """A case's descriptors and keys on the device, uploaded once for all its calls."""

    def __init__(self, case):
        self.case = case
        self.desc, self.keys = _dev(case.desc.view(np.int64)), _dev(case.keys.view(np.int32))

    def match(self, call, n_pairs=None):
        import visual_underwater_slam_amd._lib as L
        K = self.case.keys.shape[1]
        n_pairs = len(call.q) if n_pairs is None else n_pairs
        idx = torch.full((max(len(call.q), 1), K), SENTINEL, dtype=torch.int32, device="cuda")
        dist = torch.full((max(len(call.q), 1), K), SENTINEL, dtype=torch.int32, device="cuda")
        kc, q, t = _dev(call.kp_count), _dev(call.q), _dev(call.t)
        L.call("vus_hamming_match", self.desc.data_ptr(), self.keys.data_ptr(), kc.data_ptr(), K, call.H, call.W,
               q.data_ptr(), t.data_ptr(), n_pairs, *call.gate, idx.data_ptr(), dist.data_ptr(), L.current_stream_ptr())
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dist.cpu().numpy()


def _check(dev, name, i):
    """Call i of the case on the GPU: every slot written, idx and dist equal to the reference."""
    call = dev.case.calls[i]
    idx, dist = dev.match(call)
    eidx, edist = C.reference(name, i)
    assert (idx != SENTINEL).all() and (dist != SENTINEL).all(), f"{name} / {call.label}: slots left unwritten"
    bad = np.argwhere((idx != eidx) | (dist != edist))
    assert bad.size == 0, (f"{name} / {call.label}: {len(bad)} slots differ, first (pair, slot) {bad[0].tolist()}: "
                           f"got {idx[tuple(bad[0])]} / {dist[tuple(bad[0])]}, "
                           f"expected {eidx[tuple(bad[0])]} / {edist[tuple(bad[0])]}")
    return idx, dist


@pytest.mark.parametrize("K", C.COUNT_K)
def test_counts_outside_0_max_kp_on_the_matrix_core_kernel(gpu, K):
    """Counts -2^31, -5, 0, 1, K - 1, K, K + 1, K + 1000 and 2^31 - 1, each on the query list and on the train list of an
    ungated call.  The image behind an over-counted one holds exact copies of the queries, so a reader that does not clamp
    returns distance 0 at an index of K or more."""
    name = f"counts-{K}"
    dev = _Device(C.case(name))
    for i, call in enumerate(dev.case.calls):
        idx, dist = _check(dev, name, i)
        live = np.clip(call.kp_count.astype(np.int64), 0, K)
        assert (idx < live[call.t][:, None]).all()
        assert (idx[live[call.q] == 0] == -1).all() and (dist[live[call.t] == 0] == 512).all()
        over = call.kp_count[call.t].astype(np.int64) > K
        assert (dist[over & (call.q == 0)] > 0).all()       # the list itself holds no exact copy of a query


@pytest.mark.parametrize("K", C.SCAN_K)
def test_ungated_tiled_scan_above_65535_keypoints(gpu, K):
    """Train counts 1, 511, 512, 513 and 1025 around the 512-train LDS tile, 701 queries, max_dist 256 and 40, a count
    above max_kp on either side; ties across the tile boundary go to the lower index, and a train one slot past the count
    is not seen although a query holds its exact copy."""
    name = f"scan-{K}"
    dev = _Device(C.case(name))
    for i, call in enumerate(dev.case.calls[:-1]):
        idx, dist = _check(dev, name, i)
        c, md = int(call.kp_count[2]), call.gate[3]
        assert (idx[0] < c).all() and (idx[0, C.SCAN_NQ:] == -1).all() and (idx[1, c:] == -1).all()
        assert dist[0, 3] == 0 and idx[0, 3] == 0
        for k, slot in enumerate(C.SCAN_TRAIN_COUNTS):      # query 10 + k is the copy of train `slot`
            first = C.MT - 1 if slot == C.MT else slot      # trains 511 and 512 are equal
            if first < c:
                assert dist[0, 10 + k] == 0 and idx[0, 10 + k] == first
            else:
                assert dist[0, 10 + k] > 0
        if c == 1:
            assert dist[0, 4] == 256 and idx[0, 4] == (0 if md >= 256 else -1)
        if c > 900:
            assert (idx[0, 20], dist[0, 20]) == (300, 2) and (idx[0, 22], dist[0, 22]) == (700, 3)
        if c > 2 * C.MT:
            assert (idx[0, 21], dist[0, 21]) == (2 * C.MT - 1, 1)
        if c > 500 and md == 40:
            assert (dist[0, 32:90:6] == 40).all() and (idx[0, 32:90:6] >= 0).all()
            assert (dist[0, 33:90:6] == 41).all() and (idx[0, 33:90:6] == -1).all()
    idx, dist = _check(dev, name, len(dev.case.calls) - 1)
    assert idx[0, 5] == K - 1 and dist[0, 5] == 0           # the last slot of a list counted above max_kp
    assert (idx[0, 65:] == -1).all() and (idx[1] <= 0).all() and (dist[1] < 512).all()


def test_one_pair_of_lists_on_the_three_gated_kernels(gpu):
    """max_kp 300, W 64: H = 64 runs the LDS-resident kernel, 11000 the gathering one, 12288 the tiled scan.  Keypoints at
    H * W, at VUS_KEY_INVALID and at H * W + x take no part on either side although their descriptors have exact copies in
    front of them; a valid train at the last pixel does.  The three results are identical; the ungated call matches the
    same slots by their descriptors."""
    dev = _Device(C.case("gated"))
    calls, notes = dev.case.calls, dev.case.notes
    got = {call.label: _check(dev, "gated", i) for i, call in enumerate(calls)}
    for g in range(len(C.GATED_GATES)):
        for path in ("gather", "scan"):
            assert np.array_equal(got[f"{path} gate{g}"][0], got[f"rows gate{g}"][0])
            assert np.array_equal(got[f"{path} gate{g}"][1], got[f"rows gate{g}"][1])
        idx, dist = got[f"rows gate{g}"]
        outside_q, outside_t = list(notes["outside_queries"]), list(notes["outside_trains"].values())
        assert (idx[0, outside_q] == -1).all() and (dist[0, outside_q] == 512).all()
        assert (idx[1, outside_t] == -1).all() and (dist[1, outside_t] == 512).all()
        assert not np.isin(idx[0], outside_t).any() and not np.isin(idx[1], outside_q).any()
        assert not np.isin(idx[2], outside_q).any()
        assert (idx[0] < 297).all()
        q, t = notes["last_pixel"]
        assert idx[0, q] == t and dist[0, q] == 0
    idx, dist = got["ungated"]
    for q, t in {**notes["outside_queries"], **notes["outside_trains"]}.items():
        assert idx[0, q] == t and dist[0, q] == 0


@pytest.mark.parametrize("path", list(C.WORKLOAD))
def test_invalid_keys_in_the_counted_part_at_the_workload_sizes(gpu, path):
    """VUS_KEY_INVALID in the counted part of both lists, as an overflowed selection leaves it, at (2000, 720 x 640) on
    the LDS-resident kernel and at (2049, 720 x 640) on the gathering one: not a candidate of the bottom-row queries that
    hold the same descriptor."""
    name = f"workload-{path}"
    dev = _Device(C.case(name))
    K, n_inv = dev.case.keys.shape[1], dev.case.notes["n_inv"]
    for i in range(len(dev.case.calls)):
        idx, dist = _check(dev, name, i)
        assert (idx < K - n_inv).all()
        assert (idx[:, K - n_inv:] == -1).all() and (dist[:, K - n_inv:] == 512).all()
        assert (dist[:, 100:100 + n_inv] > 0).all()
        assert (dist < 512).sum() > K                       # the gate leaves real work


def test_index_tables_self_pairs_and_repeated_pairs(gpu):
    dev = _Device(C.case("tables"))
    for i, call in enumerate(dev.case.calls):
        idx, dist = _check(dev, "tables", i)
        a, b = dev.case.notes["same"]
        assert np.array_equal(idx[a], idx[b]) and np.array_equal(dist[a], dist[b])
        for p in dev.case.notes["self"]:
            n = int(call.kp_count[call.q[p]])
            assert (idx[p, :n] == np.arange(n)).all() and (dist[p, :n] == 0).all()


def test_index_tables_no_pairs_and_the_most_pairs(gpu):
    dev = _Device(C.case("many-pairs"))
    for i, call in enumerate(dev.case.calls):
        idx, dist = dev.match(call, n_pairs=0)
        assert (idx == SENTINEL).all() and (dist == SENTINEL).all()
        idx, dist = _check(dev, "many-pairs", i)
        assert len(idx) == 65535 and (idx >= 0).any() and (idx < 0).any()


def test_index_tables_one_pair_too_many_is_refused(gpu):
    import visual_underwater_slam_amd._lib as L
    dev = _Device(C.case("many-pairs"))
    call = dev.case.calls[0]
    call = call._replace(q=np.append(call.q, 0).astype(np.int32), t=np.append(call.t, 0).astype(np.int32))
    with pytest.raises(L.VusError, match=r"vus_hamming_match failed \(-1\).*n_pairs=65536 out of range \[0, 65535\]"):
        dev.match(call)
