#!/usr/bin/env python3
"""LDS-array cycles per keypoint of the tiled orientation + rBRIEF kernel (csrc/orient.hip), from the bank rules.

An LDS instruction of a wave is served in fixed lane groups; a group takes one LDS-array cycle when its lanes ask for
different banks (or for one and the same dword: a broadcast), and one cycle more for every further dword on a busy
bank.  What counts as a group and as a bank depends on the instruction:

    ds_read_u8 / ds_read_b32    2 groups of 32 lanes              bank = (byte address / 4) mod 32
    ds_read_b64                 2 groups of 32 lanes              bank = (byte address / 4) mod 64
    ds_read2_b64                two accesses, 4 groups of 16 each bank = (byte address / 4) mod 32
    ds_write_b128               8 groups of 8 lanes               bank = (byte address / 4) mod 32
    ds_write_b32                2 groups of 32 lanes              bank = (byte address / 4) mod 32

SQ_LDS_IDX_ACTIVE counts all these cycles, SQ_LDS_BANK_CONFLICT the ones beyond the first of a group.  The model lays
the kernel's three LDS access kinds over these rules:

    weights   phase A: the {moment, count} entries of a centroid piece's four dwords, 32 bytes per lane, out of the copy
              of g_disc_weight_dw_table -- 1.5 wave-loads per keypoint (TiledDiscPair), averaged over the 16 x 16 byte
              alignments of a pair of keypoints
    bytes     phase B: the 8 byte reads per lane of the 256 tests, averaged over the 30 bins and the byte alignments
    stores    phase B: the two ds_write_b128 that put the descriptor patch into LDS (and, apart, the ds_write_b32 of the
              dword column at alignments past 11)

The layout is READ from the source: the `constexpr int` constants of orient.hip (rows and entries of the weight table,
folded or not; the LDS pitch of the descriptor patch; the rows, piece columns and group size of the two dealings) and
VUS_RBRIEF_ROT of include/vus_orb_tables.h.  --source names another orient.hip (an earlier revision, say).

usage: python tools/lds_bank_model.py [--source orient.hip] [--weights-form read2_b64|b64] [--pitch BYTES]
"""
import argparse
import json
import os
import re
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "visual-underwater-slam_amd", "csrc", "orient.hip")
TABLES = os.path.join(ROOT, "include", "vus_orb_tables.h")

GROUPS = {   # instruction -> (lanes per group, bank modulus)
    "ds_read_u8": (32, 32), "ds_read_b64": (32, 64), "ds_read2_b64": (16, 32), "ds_write_b128": (8, 32), "ds_write_b32": (32, 32),
}


def header_defines(path=TABLES):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (VUS_\w+) (-?\d+)\b", open(path).read(), re.M)}


def header_array(name, path=TABLES):
    m = re.search(name + r"\[[^\]]*\] = \{(.*?)\};", open(path).read(), re.S)
    return np.array([int(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()], np.int64)


def source_constants(path=SOURCE):
    """Every `constexpr int NAME = <integer expression>;` at namespace scope of the source, evaluated in order."""
    env = dict(header_defines())
    for m in re.finditer(r"^constexpr int (\w+) = ([^;]+);", open(path).read(), re.M):
        expr = m.group(2).replace("::", "").replace("/", "//")
        try:
            env[m.group(1)] = int(eval(expr, {"__builtins__": {}}, env))   # names and integer arithmetic only
        except Exception:
            pass                                                           # not a plain integer expression: not a layout constant
    return env


def layout(path=SOURCE):
    """What the model needs of the source, by name."""
    c = source_constants(path)
    rows, pc = c["OR_ROWS"], c["OR_PC"]
    return dict(
        disc_rows=rows, disc_pc=pc,
        weight_row_entries=c.get("OR_WROW", 4 * pc),       # entries of 8 bytes per table row
        weight_folded="OR_WFOLD" in c,                      # rows r and rows - 1 - r share an entry
        weight_alignment_entries=c["OR_WTD"],               # entries per byte alignment (4 of them)
        brief_rows=c["BR_ROWS"], brief_pc=c.get("BR_PC", 3), brief_group_rows=c.get("BR_GROUP_ROWS", 4),
        brief_pitch=4 * c["BR_DW_TILED"], row_major_pitch=4 * c["BR_DW"], reach=c["BR_R"], bins=c["VUS_N_ANGLE_BINS"])


def group_cycles(addr, width, instr, active=None):
    """LDS-array cycles of one access of a wave: addr[64] byte addresses, `width` bytes per lane.  Per lane group the
    largest number of different dwords that fall on one bank; a group with no active lane takes no cycle."""
    lanes, banks = GROUPS[instr]
    total = 0
    for g in range(0, 64, lanes):
        on_bank = defaultdict(set)
        for lane in range(g, g + lanes):
            if active is not None and not active[lane]:
                continue
            for dw in range(int(addr[lane]) // 4, (int(addr[lane]) + width + 3) // 4):
                on_bank[dw % banks].add(dw)
        total += max((len(v) for v in on_bank.values()), default=0)
    return total


# ---- phase A: the weights
def disc_piece(q, L):
    c = q // L["disc_rows"]
    return q - L["disc_rows"] * c, c


def weight_entry(r, c, L):
    rr = min(r, L["disc_rows"] - 1 - r) if L["weight_folded"] else r
    return L["weight_row_entries"] * rr + 4 * c


def weight_reads(L, form="read2_b64"):
    """(cycles, conflict cycles) per keypoint of the weight reads: three wave-loads serve a pair of keypoints."""
    n_pieces = L["disc_rows"] * L["disc_pc"]
    entry = np.zeros((3, 64), np.int64)
    second = np.zeros((3, 64), bool)
    for u in range(3):
        for lane in range(64):
            p = min(lane + 64 * u, 2 * n_pieces - 1)
            second[u, lane] = p >= n_pieces
            entry[u, lane] = weight_entry(*disc_piece(p % n_pieces, L), L)
    instr = "ds_read2_b64" if form == "read2_b64" else "ds_read_b64"
    ideal_per_access = 64 // GROUPS[instr][0]
    base = lambda sh: (sh & 3) * L["weight_alignment_entries"] + 3 - (sh >> 2)
    # wave-loads 0 and 2 see one alignment each, wave-load 1 both
    one = np.zeros((3, 16))
    for u in (0, 2):
        for sh in range(16):
            one[u, sh] = sum(group_cycles(8 * (base(sh) + entry[u] + j), 8, instr) for j in range(4))
    mixed = np.zeros((16, 16))
    for sha in range(16):
        for shb in range(16):
            b = np.where(second[1], base(shb), base(sha))
            mixed[sha, shb] = sum(group_cycles(8 * (b + entry[1] + j), 8, instr) for j in range(4))
    per_pair = one[0].mean() + mixed.mean() + one[2].mean()
    ideal = 3 * 4 * ideal_per_access
    return per_pair / 2, (per_pair - ideal) / 2


# ---- phase B: the byte reads
def rotated_pattern(L):
    return header_array("VUS_RBRIEF_ROT").reshape(L["bins"], 256, 4)   # [bin, test, (x0, y0, x1, y1)]


def byte_reads(L, pitch, alignments):
    """(cycles, conflict cycles) per keypoint of the 8 ds_read_u8 per lane: test 64 w + lane reads bytes
    (reach + y) pitch + reach + a + x of the patch, a the byte alignment of the patch's first column."""
    rot, R = rotated_pattern(L), L["reach"]
    total = 0
    for k in range(L["bins"]):
        for a in range(alignments):
            for w in range(4):
                t = rot[k, 64 * w:64 * w + 64]
                for h in (0, 2):
                    total += group_cycles((R + t[:, h + 1]) * pitch + R + a + t[:, h], 1, "ds_read_u8")
    mean = total / (L["bins"] * alignments)
    return mean, mean - 8 * 2


# ---- phase B: the patch stores
def brief_piece(t, L):
    per_group = L["brief_group_rows"] * L["brief_pc"]
    g, w = divmod(t, per_group)
    return L["brief_group_rows"] * g + w % L["brief_group_rows"], w // L["brief_group_rows"]


def patch_stores(L, pitch):
    """(cycles, conflict cycles) per keypoint of the two ds_write_b128: slot lane + 64 u stores piece (r, c) at pitch r + 16 c."""
    slots = L["brief_group_rows"] * L["brief_pc"] * -(-L["brief_rows"] // L["brief_group_rows"])
    total = ideal = 0
    for u in range(2):
        addr, active = np.zeros(64, np.int64), np.zeros(64, bool)
        for lane in range(64):
            t = lane + 64 * u
            r, c = brief_piece(min(t, slots - 1), L)
            active[lane] = t < slots and r < L["brief_rows"]
            addr[lane] = pitch * min(r, L["brief_rows"] - 1) + 16 * c
        total += group_cycles(addr, 16, "ds_write_b128", active)
        ideal += sum(1 for g in range(0, 64, 8) if active[g:g + 8].any())
    return float(total), float(total - ideal)


def column_store(L, pitch, alignments=16, wide_from=12):
    """(cycles, conflict cycles) per keypoint of the dword column's ds_write_b32 (alignments past 11 only): row `lane`, byte 48."""
    addr, active = pitch * np.arange(64) + 48, np.arange(64) < L["brief_rows"]
    cyc = group_cycles(addr, 4, "ds_write_b32", active)
    share = (alignments - wide_from) / alignments
    return share * cyc, share * (cyc - 2)


def model(path=SOURCE, weights_form="read2_b64", pitch=None):
    L = layout(path)
    pitch = pitch or L["brief_pitch"]
    out = dict(layout=dict(L, brief_pitch=pitch, weights_form=weights_form))
    for name, (cyc, conf) in (("weights", weight_reads(L, weights_form)), ("bytes", byte_reads(L, pitch, 16)),
                              ("stores", patch_stores(L, pitch)), ("column", column_store(L, pitch))):
        out[name] = dict(cycles=round(cyc, 2), conflict=round(conf, 2))
    out["sum"] = dict(cycles=round(sum(out[k]["cycles"] for k in ("weights", "bytes", "stores", "column")), 2),
                      conflict=round(sum(out[k]["conflict"] for k in ("weights", "bytes", "stores", "column")), 2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--source", default=SOURCE)
    ap.add_argument("--weights-form", choices=("read2_b64", "b64"), default="read2_b64")
    ap.add_argument("--pitch", type=int, help="LDS row bytes of the descriptor patch instead of the source's")
    a = ap.parse_args()
    print(json.dumps(model(a.source, a.weights_form, a.pitch)))


if __name__ == "__main__":
    main()
