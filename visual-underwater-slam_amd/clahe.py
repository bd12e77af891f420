"""Photometric input stage: contrast-limited adaptive histogram equalisation (CLAHE) in front of
`StereoOrbFrontend.process`.

Under water, backscatter adds a veiling light and the vehicle's lamp lights a cone that falls off towards the image
border; the detector's fixed threshold finds next to nothing on such frames.  `Clahe.enhance` runs the two launches of
include/vus_clahe.h (per-tile lookup tables, then the bilinear blend of the four nearest tables) over the whole resident
batch.  It is the photometric counterpart of `rectify.StereoRectifier`; `sequence.run_sequence(..., enhancer=Clahe(H, W))`
puts it between the rectifier and the front end.  Integer arithmetic, bit-equal to its numpy statement; there is no CPU
fallback.
"""
from . import _abi

MAX_TILES, MAX_TILE_PIXELS = _abi.const("VUS_CLAHE_MAX_TILES"), _abi.const("VUS_CLAHE_MAX_TILE_PIXELS")


def clip_count(clip_limit: float, tw: int, th: int) -> int:
    """The integer clip of the C ABI from OpenCV's clipLimit: max(1, int(clip_limit * T / 256)) for clip_limit > 0, else 0
    (no clipping), in double precision."""
    if not clip_limit > 0:
        return 0
    return max(1, int(float(clip_limit) * (int(tw) * int(th)) / 256.0))


def tile_size(H: int, W: int, tiles_x: int, tiles_y: int, who: str = "clahe"):
    """(tw, th) of include/vus_clahe.h; ValueError, worded as the C entry points word it, where they refuse the call."""
    if not (1 <= H <= 32767 and 1 <= W <= 32767):
        raise ValueError(f"{who}: H={H} W={W} outside 1..32767")
    if not (1 <= tiles_x <= MAX_TILES and 1 <= tiles_y <= MAX_TILES):
        raise ValueError(f"{who}: tiles_x={tiles_x} tiles_y={tiles_y} outside 1..{MAX_TILES}")
    tw, th = -(-W // tiles_x), -(-H // tiles_y)
    if tiles_y * th - H > H - 1:
        raise ValueError(f"{who}: tiles_y={tiles_y} pads H={H} by {tiles_y * th - H} rows, reflect-101 has H - 1 = {H - 1}")
    if tiles_x * tw - W > W - 1:
        raise ValueError(f"{who}: tiles_x={tiles_x} pads W={W} by {tiles_x * tw - W} columns, reflect-101 has W - 1 = {W - 1}")
    if tw * th > MAX_TILE_PIXELS:
        raise ValueError(f"{who}: a tile of T={tw * th} pixels ({tw} x {th}) exceeds 2^22")
    return tw, th


class Clahe:
    """CLAHE of H x W uint8 images with tiles = (tiles_x, tiles_y) tiles and OpenCV's clip_limit (0: no clipping, plain
    adaptive equalisation).

    Members: tiles, clip_limit, tile_size = (tw, th), clip (the integer the kernels take), luts (uint8
    [n, tiles_y, tiles_x, 256] on the device: made on first use, re-made only when the image count grows; the first n
    tables are those of the last call), enhanced (the buffer the last enhance() without `out` wrote, or None)."""

    def __init__(self, H: int, W: int, tiles=(8, 8), clip_limit: float = 4.0):
        self.H, self.W = int(H), int(W)
        self.tiles = (int(tiles[0]), int(tiles[1]))
        self.tile_size = tile_size(self.H, self.W, self.tiles[0], self.tiles[1])
        self.clip_limit = float(clip_limit)
        if not self.clip_limit >= 0:
            raise ValueError(f"clahe: clip_limit={clip_limit} is negative")
        self.clip = clip_count(self.clip_limit, *self.tile_size)
        self._luts = self._out = None

    @property
    def luts(self):
        return self._luts

    @property
    def enhanced(self):
        return self._out

    def enhance(self, frames, out=None):
        """frames uint8 [F, 2, H, W] or [n, H, W] on the device -> the enhanced images in the same shape: vus_clahe_luts
        and vus_clahe_apply on the current stream.  Without `out` the result lives in a buffer of this object that the
        next call of the same shape reuses; out=frames works in place."""
        import torch
        from . import _lib
        _lib.require_gpu()
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()):
            raise ValueError("clahe: frames must be a contiguous uint8 tensor on the device")
        if not ((frames.dim() == 4 and frames.shape[1] == 2 or frames.dim() == 3) and tuple(frames.shape[-2:]) == (self.H, self.W)):
            raise ValueError(f"clahe: frames of shape {tuple(frames.shape)}, expected [F, 2, {self.H}, {self.W}] or "
                             f"[n, {self.H}, {self.W}]")
        n = frames.numel() // (self.H * self.W)
        if n < 1:
            raise ValueError(f"clahe: n_img={n}, needs at least one image")
        if out is None:
            if self._out is None or self._out.shape != frames.shape or self._out.device != frames.device:
                self._out = torch.empty_like(frames)
            out = self._out
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.shape == frames.shape and out.is_contiguous()
                and out.device == frames.device):
            raise ValueError("clahe: out must be a contiguous uint8 tensor of the shape and device of frames")
        if self._luts is None or self._luts.shape[0] < n or self._luts.device != frames.device:
            self._luts = torch.empty((n, self.tiles[1], self.tiles[0], 256), dtype=torch.uint8, device=frames.device)
        with torch.cuda.device(frames.device):
            st = _lib.current_stream_ptr()
            _lib.call("vus_clahe_luts", _lib.ptr(frames), n, self.H, self.W, self.W, self.tiles[0], self.tiles[1], self.clip,
                      _lib.ptr(self._luts), st)
            _lib.call("vus_clahe_apply", _lib.ptr(frames), n, self.H, self.W, self.W, _lib.ptr(self._luts), self.tiles[0],
                      self.tiles[1], _lib.ptr(out), self.W, st)
        return out
