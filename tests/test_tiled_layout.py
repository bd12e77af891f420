"""Block-tiled image planes (include/vus_tiled.h) without a GPU: the layout helpers of the front-end against the index
formula of the header, and the host-side argument checks of the tiled entry points."""
import ctypes
import os
import re

import numpy as np
import torch

from visual_underwater_slam_amd.frontend import TILE_BH, TILE_BW, tile_planes, tiled_supported, untile_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offset(y, x, W):
    """vus_tiled_offset of include/vus_tiled.h, written out."""
    return ((y // 8) * (W // 16) + x // 16) * 128 + (y % 8) * 16 + x % 16


def test_header_states_the_block_shape_the_helpers_use():
    txt = open(os.path.join(ROOT, "include", "vus_tiled.h")).read()
    assert int(re.search(r"#define VUS_TILE_BW (\d+)", txt).group(1)) == TILE_BW == 16
    assert int(re.search(r"#define VUS_TILE_BH (\d+)", txt).group(1)) == TILE_BH == 8


def test_tile_planes_matches_the_index_formula_and_round_trips():
    rng = np.random.default_rng(3)
    for H, W in ((8, 16), (96, 128), (24, 48), (720, 1280)):
        a = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
        t = tile_planes(torch.from_numpy(a)).numpy()
        assert t.shape == (2, H * W)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        off = _offset(ys, xs, W)
        assert np.array_equal(np.sort(off.ravel()), np.arange(H * W))          # a permutation of the plane
        assert np.array_equal(t[:, off], a)
        assert np.array_equal(untile_planes(torch.from_numpy(t), H, W).numpy(), a)


def test_a_block_is_one_128_byte_line():
    W = 64
    for by, bx in ((0, 0), (2, 3)):
        offs = sorted(_offset(8 * by + r, 16 * bx + c, W) for r in range(8) for c in range(16))
        assert offs == list(range(offs[0], offs[0] + 128)) and offs[0] % 128 == 0


def test_tiled_sizes():
    assert tiled_supported(720, 1280) and tiled_supported(96, 128) and tiled_supported(240, 320)
    assert not tiled_supported(100, 128) and not tiled_supported(96, 130) and not tiled_supported(360, 642)


def test_tiled_entry_points_reject_bad_arguments_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p16 = ctypes.c_void_p(1 << 20)
    # sizes that are not whole 16 x 8 blocks
    rc = lib.vus_fast_detect_adaptive_tiled(p16, 1, 100, 128, 128, p16, 31, p16, p16, p16, 4096, p16, None)
    assert rc == -1 and b"W % 16" in lib.vus_last_error()
    rc = lib.vus_orient_rbrief_tiled(p16, p16, 1, 96, 130, p16, p16, 100, None, p16, p16, None)
    assert rc == -1 and b"W % 16" in lib.vus_last_error()
    # plane pointers: null, misaligned
    rc = lib.vus_fast_detect_adaptive_tiled(p16, 1, 96, 128, 128, p16, 31, None, p16, p16, 4096, p16, None)
    assert rc == -1 and b"null" in lib.vus_last_error()
    rc = lib.vus_orient_rbrief_tiled(p16, ctypes.c_void_p((1 << 20) + 8), 1, 96, 128, p16, p16, 100, None, p16, p16, None)
    assert rc == -1 and b"aligned" in lib.vus_last_error()
    # the rest as in the row-major entry points
    rc = lib.vus_orient_rbrief_tiled(p16, p16, 1, 96, 128, None, p16, 100, None, p16, p16, None)
    assert rc == -1 and b"null" in lib.vus_last_error()
    rc = lib.vus_fast_detect_adaptive_tiled(p16, 1, 96, 128, 128, None, 31, p16, p16, p16, 4096, p16, None)
    assert rc == -1 and b"null" in lib.vus_last_error()
