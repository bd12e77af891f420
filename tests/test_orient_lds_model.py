"""tools/lds_bank_model.py: the LDS bank model of the tiled orientation + rBRIEF kernel, anchored at a measured counter, and
the bounds it sets on the layout that csrc/orient.hip has now (no GPU needed).

The kernel was bound by its LDS array (profiles/orient_lds_r10.md): the weight table's row stride and the descriptor
patch's row pitch decide how many lanes of a group meet on one bank.  The model reads both from the source, so a later
change of either that brings the conflicts back fails here."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_bank_model as M   # noqa: E402

KEYPOINTS_PER_LAUNCH = 400 * 2000          # profiles/pmc_orient_r04.txt: bench.py --frames 200, 2000 keypoints per image


@pytest.fixture(scope="module")
def tree_layout():
    return M.layout()


def _r04_counter(name):
    txt = open(os.path.join(ROOT, "profiles", "pmc_orient_r04.txt")).read()
    return float(re.search(r"^\s*" + name + r"\s+n=\s*\d+\s+mean=(\S+)", txt, re.M).group(1))


def test_byte_read_conflicts_of_40_byte_rows_equal_the_round_4_counter(tree_layout):
    """The row-major kernel of round 4 had no other LDS conflicts than those of its byte reads on 40-byte patch rows (four
    dword alignments): SQ_LDS_BANK_CONFLICT per keypoint is what the model must give, within 2 %."""
    measured = _r04_counter("SQ_LDS_BANK_CONFLICT") / KEYPOINTS_PER_LAUNCH
    pitch = tree_layout["row_major_pitch"]
    assert pitch == 40
    _, conflict = M.byte_reads(tree_layout, pitch, 4)
    print(f"byte-read conflicts, 40-byte rows: model {conflict:.3f}, measured {measured:.3f} cycles per keypoint")
    assert abs(conflict - measured) <= 0.02 * measured


def test_weight_reads_of_the_tree_cost_at_most_36_cycles(tree_layout):
    """ds_read2_b64 form: 3 instructions of two accesses in 4 lane groups per keypoint are 24 cycles; what lies above are
    the groups that span two piece columns."""
    cycles, conflict = M.weight_reads(tree_layout, "read2_b64")
    print(f"weight reads: {cycles:.2f} cycles per keypoint, {conflict:.2f} of them conflicts")
    assert cycles - conflict == pytest.approx(24.0)
    assert cycles <= 36.0


def test_byte_reads_of_the_tree_cost_at_most_52_cycles(tree_layout):
    cycles, conflict = M.byte_reads(tree_layout, tree_layout["brief_pitch"], 16)
    print(f"byte reads, {tree_layout['brief_pitch']}-byte rows: {cycles:.2f} cycles per keypoint, {conflict:.2f} of them conflicts")
    assert cycles - conflict == pytest.approx(16.0)
    assert cycles <= 52.0
