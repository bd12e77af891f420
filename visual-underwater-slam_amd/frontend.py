"""Host side of the stereo ORB front-end: the MI355X replacement of the reference's external
image-processor nodelet.

Interface mirrored: the nodelet is configured by the ROS parameters of
/root/reference/launch/stereo.launch:37-47 (`fast_threshold`, `stereo_threshold`, ...) and publishes
`gtsam_vio/CameraMeasurement` messages whose `features[].id, u0, v0, u1, v1` fields are what
/root/reference/batch.py:149-154 reads.  `ImageProcessorParams` carries those parameter names,
`StereoOrbFrontend.process()` runs the kernels on a whole resident batch of stereo frames, and
`camera_measurements()` emits records of exactly that message shape.

Python here only owns buffers and launches: every number is produced by libvus_hip.so.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _abi, _lib, synth


TILE_BW, TILE_BH = 16, 8   # block-tiled planes (include/vus_tiled.h): 16 x 8-pixel blocks of 128 bytes, raster order


def tiled_supported(H: int, W: int) -> bool:
    """The tiled entry points take whole blocks only."""
    return H % TILE_BH == 0 and W % TILE_BW == 0


def tile_planes(planes: torch.Tensor) -> torch.Tensor:
    """[n, H, W] row-major -> [n, H * W] block-tiled (vus_tiled_offset of include/vus_tiled.h)."""
    n, H, W = planes.shape
    return (planes.reshape(n, H // TILE_BH, TILE_BH, W // TILE_BW, TILE_BW).permute(0, 1, 3, 2, 4)
            .reshape(n, H * W).contiguous())


def untile_planes(tiled: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[n, H * W] block-tiled -> [n, H, W] row-major: the inverse of tile_planes."""
    n = tiled.shape[0]
    return (tiled.reshape(n, H // TILE_BH, W // TILE_BW, TILE_BH, TILE_BW).permute(0, 1, 3, 2, 4)
            .reshape(n, H, W).contiguous())


@dataclass
class ImageProcessorParams:
    """Parameter names follow launch/stereo.launch:37-47 where the reference has one."""
    fast_threshold: int = 10       # stereo.launch:43
    stereo_threshold: int = 5      # stereo.launch:47 -- |v_left - v_right| gate in pixels
    max_features: int = 2000       # BASELINE.json configs[1]: 2000 keypoints per image
    border: int = 31               # ORB edge threshold (31x31 patch)
    min_disparity: int = 0         # x_left - x_right gate of the stereo matcher
    max_disparity: int = 128
    stereo_max_distance: int = 64  # Hamming acceptance thresholds
    track_max_distance: int = 64
    cand_cap: int = 0              # candidate slots per image before top-K selection; 0 = sized from the image:
                                   # max(32768, H*W/16) -- strict 3x3 NMS leaves at most H*W/4 candidates, the
                                   # corner-dense bench texture ~H*W/37; an overflow is never silent (check_overflow)
    grid_row: int = 0              # stereo.launch:36-39 -- with grid_max_feature_num > 0 every cell of the
    grid_col: int = 0              # grid_row x grid_col grid keeps its grid_max_feature_num best corners
    grid_max_feature_num: int = 0  # (the nodelet's values: 3 x 4 cells, 4 per cell); 0 = global top max_features
    cross_check: bool = False      # keep a match only if it is mutual (query <-> train swapped gives it back)
    n_levels: int = 1              # ORB scale pyramid: 1 = single level; 8 with scale_factor 1.2 = Rublee et al.
    scale_factor: float = 1.2
    adaptive_fast: bool = True     # detect at a per-image threshold estimated from a sample of tiles and verified on the
                                   # device (vus_fast_threshold_estimate / _detect_adaptive / _detect_retry): the SAME
                                   # max_features keypoints as detection at fast_threshold, bit for bit, at a fraction
                                   # of the exact-score work.  Applies wherever a global top-K follows (single level, or
                                   # every pyramid level with its quota); grid bucketing needs every candidate: off there
    ransac_threshold: float = 0.0  # stereo.launch:46 (the nodelet's value: 3) -- two-point RANSAC with the inter-frame
                                   # rotation on the temporal matches, inlier distance in pixels
                                   # (StereoOrbFrontend.reject_track_outliers, include/vus_ransac.h); 0 = off
    ransac_hypotheses: int = 256   # models tried per frame pair
    ransac_seed: int = synth.SEED  # seed of their two-match samples
    fast_sample_stride: int = 32   # every 32nd 128 x 24 tile is sampled (3 % of the image: ~90 survivors decide, 3.9 sigma
                                   # from a wrong answer at the 1.75x margin -- and a wrong answer only costs that image a retry)


def pyramid_layout(H: int, W: int, max_features: int, n_levels: int, scale_factor: float):
    """Level sizes and per-level keypoint quotas of the ORB pyramid (ORB paper sec. 6.1; the quota rule is the
    usual geometric split: level l gets a share proportional to scale_factor**-l, the last level the remainder)."""
    sizes = [(int(round(H / scale_factor ** l)), int(round(W / scale_factor ** l))) for l in range(n_levels)]
    if n_levels == 1:
        return sizes, [max_features]
    f = 1.0 / scale_factor
    nd = max_features * (1.0 - f) / (1.0 - f ** n_levels)
    quotas, total = [], 0
    for _ in range(n_levels - 1):
        q = int(round(nd))
        quotas.append(q)
        total += q
        nd *= f
    quotas.append(max(max_features - total, 0))
    return sizes, quotas


def default_camera(H: int, W: int) -> np.ndarray:
    """(fx, fy, cx, cy) of batch.py:111's calibration -- given for the 1920 x 1080 frame -- in pixels of an H x W image:
    pixel x is the ray through u = x * 1920 / W, the mapping synth.scene_sequence and BatchSequence.cam_array assume."""
    fx, fy, cx, cy = synth.INTRINSIC
    sx, sy = W / float(synth.RES_X), H / float(synth.RES_Y)
    return np.array([fx * sx, fy * sy, cx * sx, cy * sy], dtype=np.float64)


@dataclass
class Feature:
    """One entry of CameraMeasurement.features (batch.py:149-154)."""
    id: int
    u0: float
    v0: float
    u1: float
    v1: float


@dataclass
class CameraMeasurement:
    features: List[Feature] = field(default_factory=list)


@dataclass
class PairPoses:
    """Device tensors of one StereoOrbFrontend.relative_poses() call (vus_stereo_pair_pose, include/vus_loop.h)."""
    T_ab: torch.Tensor            # f64 [n_pairs, 12]  flat12 of T_a^-1 T_b, camera frames
    JtJ: torch.Tensor             # f64 [n_pairs, 6, 6]  normal matrix of the refit over the final inliers, (omega, v), pixels
    rss: torch.Tensor             # f64 [n_pairs]  sum of squared residuals over the final inliers, pixels^2
    info: torch.Tensor            # int32 [n_pairs, 6]  (n, best k, its count, final inliers, status, refit rounds)
    match_idx_out: torch.Tensor   # int32 [n_pairs, K]  the matches that are final inliers, -1 otherwise
    pair_a: Optional[torch.Tensor] = None      # int32 [n_pairs]  the frame numbers the call was made with (what
    pair_b: Optional[torch.Tensor] = None      # refine_relative_poses() runs its second stage on)


@dataclass
class PairBundle:
    """Device tensors of one StereoOrbFrontend.refine_relative_poses() call (vus_stereo_pair_bundle,
    include/vus_pair_bundle.h): the two-view refit behind relative_poses()."""
    T_ab: torch.Tensor            # f64 [n_pairs, 12]  flat12 of T_a^-1 T_b, camera frames
    S: torch.Tensor               # f64 [n_pairs, 6, 6]  reduced normal matrix of the pose, (omega, v), whitened
    chi2: torch.Tensor            # f64 [n_pairs]  sum of whitened squared residuals over the final active points (6 each)
    points: torch.Tensor          # f64 [n_pairs, K, 3]  refined point of every final active slot in camera a, zero elsewhere
    info: torch.Tensor            # int32 [n_pairs, 6]  (n, active in round 0, final active, status, rounds, 0)
    match_idx_out: torch.Tensor   # int32 [n_pairs, K]  the matches of the final active points, -1 otherwise


class FrontendResult:
    """Device tensors produced by one process() call (views into the front-end's workspace)."""

    def __init__(self, fe, n_frames):
        F = n_frames
        self.n_frames = F
        self.W = fe.W
        self.H = fe.H
        self.kp_keys = fe.kp_keys[:2 * F]
        self.kp_count = fe.kp_count[:2 * F]
        self.desc = fe.desc[:2 * F]
        self.angle = fe.angle[:2 * F]
        self.cand_count = fe.cand_count[:2 * F]
        self.stereo_idx = fe.match_idx[:F]
        self.stereo_dist = fe.match_dist[:F]
        self.kp_level = fe.kp_level[:2 * F] if fe.kp_level is not None else None       # pyramid mode only
        self.kp_xy_q4 = fe.kp_xy_q4[:2 * F] if fe.kp_xy_q4 is not None else None       # level-0 position, 1/16 px
        self.track_idx = fe.match_idx[fe.max_frames:fe.max_frames + max(F - 1, 0)]
        self.track_dist = fe.match_dist[fe.max_frames:fe.max_frames + max(F - 1, 0)]

    def keypoints_xy_score(self):
        """Decode keys -> (x, y, score) int32 tensors [2F, K]; unused slots give score -1."""
        k = self.kp_keys.to(torch.int64) & 0xFFFFFFFF
        pos = k & 0xFFFFFF
        score = 255 - (k >> 24)
        valid = k != 0xFFFFFFFF
        y = torch.div(pos, self.W, rounding_mode="floor")
        x = pos - y * self.W
        score = torch.where(valid, score, torch.full_like(score, -1))
        return x.to(torch.int32), y.to(torch.int32), score.to(torch.int32)


class StereoOrbFrontend:
    """Batched stereo ORB: detect + describe both images of every frame, match left->right under
    the epipolar gate and left(t)->left(t+1) for tracks.  All buffers are allocated once here."""

    def __init__(self, H: int, W: int, max_frames: int, params: Optional[ImageProcessorParams] = None,
                 device: str = "cuda:0"):
        _lib.require_gpu()
        _lib.load()
        self.p = params or ImageProcessorParams()
        if self.p.cand_cap <= 0:
            import dataclasses
            self.p = dataclasses.replace(self.p, cand_cap=max(32768, (int(H) * int(W)) // 16))
        self.stage_hook = None      # optional callable(name), called on the launch stream after every stage of
                                    # process() (bench.py records HIP events there); None = no overhead
        if self.p.grid_max_feature_num > 0:
            assert self.p.grid_row >= 1 and self.p.grid_col >= 1 and self.p.n_levels == 1, \
                "grid bucketing needs grid_row, grid_col >= 1 and a single pyramid level"
        self.H, self.W, self.max_frames = int(H), int(W), int(max_frames)
        self.device = torch.device(device)
        n_img, K, cap = 2 * self.max_frames, self.p.max_features, self.p.cand_cap
        dev = self.device
        # the single-level adaptive path keeps the image and its smoothing block-tiled (include/vus_tiled.h): the
        # orientation stage's patches then touch ~half the 128-byte lines.  `blur` stays a row-major [n, H, W] tensor
        # on demand (a de-tiled copy, made when read).  Other paths, and sizes that are not whole 16 x 8 blocks, stay
        # row-major.
        self.tiled = bool(self.p.n_levels == 1 and self.p.adaptive_fast and self.p.grid_max_feature_num <= 0
                          and tiled_supported(self.H, self.W))
        if self.tiled:
            self.blur_tiled = torch.empty((n_img, H * W), dtype=torch.uint8, device=dev)
            self.img_tiled = torch.empty((n_img, H * W), dtype=torch.uint8, device=dev)
            self._blur = None
        else:
            self._blur = torch.empty((n_img, H, W), dtype=torch.uint8, device=dev)
        self.cand_keys = torch.empty((n_img, cap), dtype=torch.int32, device=dev)
        self.cand_count = torch.zeros((n_img,), dtype=torch.int32, device=dev)
        self.kp_keys = torch.empty((n_img, K), dtype=torch.int32, device=dev)
        self.kp_count = torch.zeros((n_img,), dtype=torch.int32, device=dev)
        self.desc = torch.empty((n_img, K, 4), dtype=torch.int64, device=dev)
        self.angle = torch.empty((n_img, K), dtype=torch.uint8, device=dev)
        # the schedule of the orientation + rBRIEF launch: every image's keypoint slots grouped by 64 x 64-pixel cell
        # (vus_orient_order; a schedule only -- outputs are indexed by keypoint); images of more than 1024 cells go unordered
        self.kp_order = torch.empty((n_img, K), dtype=torch.int32, device=dev)
        # rows [0, F): stereo pairs; rows [max_frames, max_frames + F - 1): temporal pairs
        self.match_idx = torch.empty((2 * self.max_frames, K), dtype=torch.int32, device=dev)
        self.match_dist = torch.empty((2 * self.max_frames, K), dtype=torch.int32, device=dev)
        f = torch.arange(self.max_frames, dtype=torch.int32, device=dev)
        self.stereo_q, self.stereo_t = (2 * f).contiguous(), (2 * f + 1).contiguous()
        self.track_q, self.track_t = (2 * f).contiguous(), (2 * f + 2).contiguous()
        self.kp_level = self.kp_xy_q4 = None
        self.levels = None
        # sticky device-side maximum of the per-image candidate counts since the last check_overflow(): a
        # process(check=False) call that overflowed cand_cap is still reported by the next check
        self.cand_max_seen = torch.zeros((1,), dtype=torch.int32, device=dev)
        # per pyramid level the top-K is the level's quota: the same argument holds level by level
        self.adaptive = bool(self.p.adaptive_fast and self.p.grid_max_feature_num <= 0)
        if self.adaptive:
            self.fast_hist = torch.zeros((n_img, 256), dtype=torch.int32, device=dev)
            self.fast_thr = torch.zeros((n_img,), dtype=torch.int32, device=dev)      # the thresholds of the last process()
            self.fast_retry_list = torch.zeros((n_img,), dtype=torch.int32, device=dev)
            self.fast_retry_count = torch.zeros((1,), dtype=torch.int32, device=dev)  # images the check sent back to fast_threshold
        if self.p.cross_check:   # backward pairings (same row layout as match_idx)
            self.rev_idx = torch.empty((2 * self.max_frames, K), dtype=torch.int32, device=dev)
            self.rev_dist = torch.empty((2 * self.max_frames, K), dtype=torch.int32, device=dev)
        if self.p.n_levels > 1:
            # per-level workspaces: image (levels >= 1), smoothed image, keys, descriptors
            sizes, quotas = pyramid_layout(H, W, K, self.p.n_levels, self.p.scale_factor)
            assert all(h >= 2 * self.p.border + 8 and w >= 2 * self.p.border + 8 for h, w in sizes), \
                "pyramid level smaller than the detector border"
            self.kp_level = torch.zeros((n_img, K), dtype=torch.uint8, device=dev)
            self.kp_xy_q4 = torch.zeros((n_img, K, 2), dtype=torch.int32, device=dev)
            self.levels = []
            for l, ((h, w), q) in enumerate(zip(sizes, quotas)):
                q = max(q, 1)
                self.levels.append(dict(
                    H=h, W=w, quota=q,
                    img=None if l == 0 else torch.empty((n_img, h, w), dtype=torch.uint8, device=dev),
                    blur=self._blur if l == 0 else torch.empty((n_img, h, w), dtype=torch.uint8, device=dev),
                    keys=torch.empty((n_img, q), dtype=torch.int32, device=dev),
                    count=torch.zeros((n_img,), dtype=torch.int32, device=dev),
                    desc=torch.empty((n_img, q, 4), dtype=torch.int64, device=dev),
                    angle=torch.empty((n_img, q), dtype=torch.uint8, device=dev)))

    def process(self, images: torch.Tensor, check: bool = True) -> FrontendResult:
        """images: uint8 [F, 2, H, W] on the GPU (index 1: 0 = left / cam0, 1 = right / cam1).
        Asynchronous on the current stream unless `check` (which reads the overflow counters)."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous()
        F = images.shape[0]
        assert images.shape[1:] == (2, self.H, self.W) and 1 <= F <= self.max_frames
        p, H, W, K = self.p, self.H, self.W, self.p.max_features
        n_img = 2 * F
        st = _lib.current_stream_ptr()
        ptr = _lib.ptr
        mark = self.stage_hook or (lambda name: None)
        mark("begin")
        if self.levels is None:
            self.cand_count[:n_img].zero_()
            if self.adaptive:
                _lib.call("vus_fast_threshold_estimate", ptr(images), n_img, H, W, W, p.fast_threshold, p.border, K,
                          p.fast_sample_stride, ptr(self.fast_hist), ptr(self.fast_thr), st)
                mark("fast_threshold")
                if self.tiled:   # both planes depend on the images only: complete before any retry
                    _lib.call("vus_fast_detect_adaptive_tiled", ptr(images), n_img, H, W, W, ptr(self.fast_thr), p.border,
                              ptr(self.blur_tiled), ptr(self.img_tiled), ptr(self.cand_keys), p.cand_cap,
                              ptr(self.cand_count), st)
                else:
                    _lib.call("vus_fast_detect_adaptive", ptr(images), n_img, H, W, W, ptr(self.fast_thr), p.border,
                              ptr(self._blur), ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), st)
                _lib.call("vus_fast_detect_retry", ptr(images), n_img, H, W, W, p.fast_threshold, ptr(self.fast_thr), K,
                          p.border, ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), ptr(self.fast_retry_list),
                          ptr(self.fast_retry_count), st)
            else:
                _lib.call("vus_fast_detect", ptr(images), n_img, H, W, W, p.fast_threshold, p.border,
                          ptr(self._blur), ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), st)
            mark("fast_detect")
            if p.grid_max_feature_num > 0:
                _lib.call("vus_select_grid", ptr(self.cand_keys), ptr(self.cand_count), n_img, p.cand_cap, H, W,
                          p.grid_row, p.grid_col, p.grid_max_feature_num, K, ptr(self.kp_keys), ptr(self.kp_count), st)
            else:
                _lib.call("vus_select_topk", ptr(self.cand_keys), ptr(self.cand_count), n_img, p.cand_cap, K,
                          ptr(self.kp_keys), ptr(self.kp_count), st)
            mark("select_topk")
            if self.tiled:
                self._orient_tiled(n_img, st)
            else:
                self._orient(ptr(images), ptr(self._blur), n_img, H, W, ptr(self.kp_keys), ptr(self.kp_count), K,
                             ptr(self.desc), ptr(self.angle), st)
            mark("orient_rbrief")
        else:
            self._process_pyramid(images, n_img, st)
            mark("pyramid_detect_describe")
        _lib.call("vus_hamming_match", ptr(self.desc), ptr(self.kp_keys), ptr(self.kp_count), K, H, W,
                  ptr(self.stereo_q), ptr(self.stereo_t), F, p.stereo_threshold, p.min_disparity,
                  p.max_disparity, p.stereo_max_distance, ptr(self.match_idx), ptr(self.match_dist), st)
        mark("hamming_stereo")
        if F > 1:
            _lib.call("vus_hamming_match", ptr(self.desc), ptr(self.kp_keys), ptr(self.kp_count), K, H, W,
                      ptr(self.track_q), ptr(self.track_t), F - 1, -1, 0, 0, p.track_max_distance,
                      ptr(self.match_idx[self.max_frames:]), ptr(self.match_dist[self.max_frames:]), st)
        mark("hamming_track")
        if p.cross_check:
            # backward pairings: right -> left under the mirrored disparity gate, left(t+1) -> left(t)
            _lib.call("vus_hamming_match", ptr(self.desc), ptr(self.kp_keys), ptr(self.kp_count), K, H, W,
                      ptr(self.stereo_t), ptr(self.stereo_q), F, p.stereo_threshold, -p.max_disparity,
                      -p.min_disparity, p.stereo_max_distance, ptr(self.rev_idx), ptr(self.rev_dist), st)
            _lib.call("vus_cross_check", ptr(self.match_idx), ptr(self.rev_idx), F, K, ptr(self.match_idx), st)
            if F > 1:
                _lib.call("vus_hamming_match", ptr(self.desc), ptr(self.kp_keys), ptr(self.kp_count), K, H, W,
                          ptr(self.track_t), ptr(self.track_q), F - 1, -1, 0, 0, p.track_max_distance,
                          ptr(self.rev_idx[self.max_frames:]), ptr(self.rev_dist[self.max_frames:]), st)
                _lib.call("vus_cross_check", ptr(self.match_idx[self.max_frames:]), ptr(self.rev_idx[self.max_frames:]),
                          F - 1, K, ptr(self.match_idx[self.max_frames:]), st)
            mark("cross_check")
        if self.levels is None:   # two tiny device ops, asynchronous: keeps an overflow visible to a later check
            torch.maximum(self.cand_max_seen, self.cand_count[:n_img].max().reshape(1), out=self.cand_max_seen)
        mark("end")
        if check:
            self.check_overflow(n_img)
        return FrontendResult(self, F)

    def _process_pyramid(self, images, n_img, st):
        """Detect / select / describe on every level, then merge level-major into the per-image lists."""
        p, K, ptr = self.p, self.p.max_features, _lib.ptr
        self.kp_count[:n_img].zero_()
        self.kp_keys[:n_img].fill_(_abi.const("VUS_KEY_INVALID") - (1 << 32))        # the uint32 pattern in int32 storage
        self.pyr_cand_max = torch.zeros((1,), dtype=torch.int32, device=self.device)
        prev = images
        for l, L in enumerate(self.levels):
            h, w = L["H"], L["W"]
            if l > 0:
                P = self.levels[l - 1]
                _lib.call("vus_resize_bilinear", ptr(prev), n_img, P["H"], P["W"], P["W"], ptr(L["img"]), h, w, w, st)
                prev = L["img"]
            self.cand_count[:n_img].zero_()
            if self.adaptive:
                _lib.call("vus_fast_threshold_estimate", ptr(prev), n_img, h, w, w, p.fast_threshold, p.border, L["quota"],
                          p.fast_sample_stride, ptr(self.fast_hist), ptr(self.fast_thr), st)
                _lib.call("vus_fast_detect_adaptive", ptr(prev), n_img, h, w, w, ptr(self.fast_thr), p.border, ptr(L["blur"]),
                          ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), st)
                _lib.call("vus_fast_detect_retry", ptr(prev), n_img, h, w, w, p.fast_threshold, ptr(self.fast_thr), L["quota"],
                          p.border, ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), ptr(self.fast_retry_list),
                          ptr(self.fast_retry_count), st)
            else:
                _lib.call("vus_fast_detect", ptr(prev), n_img, h, w, w, p.fast_threshold, p.border, ptr(L["blur"]),
                          ptr(self.cand_keys), p.cand_cap, ptr(self.cand_count), st)
            torch.maximum(self.pyr_cand_max, self.cand_count[:n_img].max().reshape(1), out=self.pyr_cand_max)
            _lib.call("vus_select_topk", ptr(self.cand_keys), ptr(self.cand_count), n_img, p.cand_cap, L["quota"],
                      ptr(L["keys"]), ptr(L["count"]), st)
            self._orient(ptr(prev), ptr(L["blur"]), n_img, h, w, ptr(L["keys"]), ptr(L["count"]), L["quota"], ptr(L["desc"]),
                         ptr(L["angle"]), st)
            _lib.call("vus_pyramid_append", ptr(L["keys"]), ptr(L["count"]), ptr(L["desc"]), ptr(L["angle"]), n_img,
                      L["quota"], h, w, l, self.H, self.W, K, ptr(self.kp_keys), ptr(self.kp_count), ptr(self.desc),
                      ptr(self.angle), ptr(self.kp_level), ptr(self.kp_xy_q4), st)

    def _orient(self, img_p, blur_p, n_img, h, w, keys_p, count_p, k, desc_p, angle_p, st):
        """Orientation + rBRIEF of n_img images of h x w pixels with k keypoint slots each, in the cell-grouped order."""
        if ((h + 63) // 64) * ((w + 63) // 64) <= 1024:
            _lib.call("vus_orient_order", keys_p, count_p, n_img, k, h, w, _lib.ptr(self.kp_order), st)
            _lib.call("vus_orient_rbrief_ordered", img_p, blur_p, n_img, h, w, w, keys_p, count_p, k, _lib.ptr(self.kp_order),
                      desc_p, angle_p, st)
        else:
            _lib.call("vus_orient_rbrief", img_p, blur_p, n_img, h, w, w, keys_p, count_p, k, desc_p, angle_p, st)

    def _orient_tiled(self, n_img, st):
        """_orient of the single-level path on the block-tiled planes of vus_fast_detect_adaptive_tiled."""
        H, W, K, ptr = self.H, self.W, self.p.max_features, _lib.ptr
        order = None
        if ((H + 63) // 64) * ((W + 63) // 64) <= 1024:
            _lib.call("vus_orient_order", ptr(self.kp_keys), ptr(self.kp_count), n_img, K, H, W, ptr(self.kp_order), st)
            order = ptr(self.kp_order)
        _lib.call("vus_orient_rbrief_tiled", ptr(self.img_tiled), ptr(self.blur_tiled), n_img, H, W, ptr(self.kp_keys),
                  ptr(self.kp_count), K, order, ptr(self.desc), ptr(self.angle), st)

    @property
    def blur(self) -> torch.Tensor:
        """The 7 x 7 smoothing of the images of the last process(), row-major [n_img, H, W] (the full-resolution
        level).  On the tiled path a de-tiled copy, made when read."""
        if self.tiled:
            return untile_planes(self.blur_tiled, self.H, self.W)
        return self._blur

    def check_overflow(self, n_img=None):
        """Raises if any image since the last check produced more FAST candidates than cand_cap (one device
        read: synchronises the stream)."""
        if self.levels is not None:
            worst = int(self.pyr_cand_max.item())
            if worst > self.p.cand_cap:
                raise _lib.VusError(f"FAST produced {worst} candidates in one pyramid level, more than cand_cap="
                                    f"{self.p.cand_cap}: raise ImageProcessorParams.cand_cap")
            return
        worst = int(self.cand_max_seen.item())
        self.cand_max_seen.zero_()
        if worst > self.p.cand_cap:
            raise _lib.VusError(f"FAST produced {worst} candidates in one image, more than cand_cap="
                                f"{self.p.cand_cap}: raise ImageProcessorParams.cand_cap")

    # ------------------------------------------------------------------------------------------
    def refine_stereo(self, res: FrontendResult, images: torch.Tensor, half_win: int = 5, search: int = 5):
        """Sub-pixel disparity of every stereo match of `res` (vus_stereo_refine, include/vus_subpixel.h): a SAD search of
        +-search columns with a (2 half_win + 1)^2 window around the matched right keypoint, on the left keypoint's row, and
        an equiangular fit of the minimum.  process() keeps no images: `images` is the tensor it was given, uint8
        [F, 2, H, W] on the GPU.  In pyramid mode the search runs on these level-0 images at the keys' integer level-0
        positions, whatever level a keypoint was found on.  Returns (disp_q8 int32 [F,K]: x_left - x_right in 1/256 px, 0
        where there is no match; status uint8 [F,K]: 0 refined, 1 minimum at the edge of the search (the integer disparity
        is kept), 255 no match).  Asynchronous on the current stream."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous()
        F, K = res.n_frames, self.p.max_features
        assert tuple(images.shape) == (F, 2, self.H, self.W), "images: the [F, 2, H, W] tensor process() was given"
        disp = torch.empty((F, K), dtype=torch.int32, device=self.device)
        status = torch.empty((F, K), dtype=torch.uint8, device=self.device)
        ptr = _lib.ptr
        _lib.call("vus_stereo_refine", ptr(images), F, self.H, self.W, self.W, ptr(res.stereo_idx), ptr(res.kp_keys),
                  ptr(res.kp_count), K, int(half_win), int(search), ptr(disp), ptr(status), _lib.current_stream_ptr())
        return disp, status

    def _check_disparity(self, res: FrontendResult, disparity: torch.Tensor):
        assert disparity.dtype == torch.int32 and disparity.is_cuda and disparity.is_contiguous() and \
            tuple(disparity.shape) == (res.n_frames, self.p.max_features), "disparity: int32 [F, K] on the device (refine_stereo)"

    def feature_tracks(self, res: FrontendResult, disparity: Optional[torch.Tensor] = None):
        """GPU CameraMeasurement emitter (vus_track_ids): returns (ids int64 [F,K], feats f64 [F,K,4],
        n_ids).  ids[f,i] >= 0 marks a published feature of frame f with persistent id; feats holds its
        (u0, v0, u1, v1) in the normalised convention that batch.py:152-154 maps back to pixels.
        disparity: refine_stereo()'s disp_q8; where ids >= 0 the right column becomes xr = (256 xl - disp_q8) / 256.0
        (exact in f64) and u1 = 2.0 * xr / W - 1.0, the kernel's own formula: 256 (xl - xr) gives today's bits."""
        F, K = res.n_frames, self.p.max_features
        dev = self.device
        ids = torch.empty((F, K), dtype=torch.int64, device=dev)
        feats = torch.empty((F, K, 4), dtype=torch.float64, device=dev)
        n_ids = torch.zeros((1,), dtype=torch.int64, device=dev)
        ptr = _lib.ptr
        _lib.call("vus_track_ids", ptr(res.stereo_idx), ptr(res.track_idx) if F > 1 else None, ptr(res.kp_keys),
                  ptr(res.kp_count), F, K, self.H, self.W, ptr(ids), ptr(feats), ptr(n_ids),
                  _lib.current_stream_ptr())
        if disparity is not None:
            self._check_disparity(res, disparity)
            pos = res.kp_keys[0:2 * F:2].to(torch.int64) & 0xFFFFFF
            xl = pos - torch.div(pos, self.W, rounding_mode="floor") * self.W
            xr = (256 * xl - disparity.to(torch.int64)).to(torch.float64) / 256.0
            # W as a device tensor: torch turns a division by a host scalar into a multiplication by its inverse
            w = torch.tensor(float(self.W), dtype=torch.float64, device=self.device)
            feats[:, :, 2] = torch.where(ids >= 0, 2.0 * xr / w - 1.0, feats[:, :, 2])
        return ids, feats, int(n_ids.item())

    def reject_track_outliers(self, res: FrontendResult, rot: torch.Tensor, cam=None, threshold_px: Optional[float] = None):
        """The nodelet's two-point RANSAC (stereo.launch:46; vus_two_point_ransac) on the temporal matches of `res`, IN
        PLACE: a left(t) -> left(t+1) match off the epipolar line that the known rotation and the best two-match model
        give becomes -1 in res.track_idx, so feature_tracks() / camera_measurements() called afterwards never join
        the two keypoints under one id.  rot: f64 [F-1, 9] device tensor, row-major R_cur_prev of every frame pair
        (a ray of camera t into camera t+1: R_{t+1}^T R_t of the world-from-camera rotations, e.g. the transpose of
        PreintegratedImuMeasurements.deltaRij()).  cam: (fx, fy, cx, cy) in pixels of this H x W image, default
        default_camera(H, W).  The inlier distance is threshold_px, default ImageProcessorParams.ransac_threshold;
        hypotheses and seed come from the parameters.  Returns info int32 [F-1, 4] on the device: (matches, survivors,
        winning hypothesis or -1, matches explained by the rotation alone) per pair.  A no-op for one frame."""
        F, K = res.n_frames, self.p.max_features
        if F < 2:
            return torch.zeros((0, 4), dtype=torch.int32, device=self.device)
        thr = float(self.p.ransac_threshold if threshold_px is None else threshold_px)
        assert rot.dtype == torch.float64 and rot.is_cuda and rot.is_contiguous() and tuple(rot.shape) == (F - 1, 9), \
            "rot: f64 [F-1, 9] on the device"
        cam_h = np.ascontiguousarray(default_camera(self.H, self.W) if cam is None else
                                     (cam.detach().cpu().numpy() if isinstance(cam, torch.Tensor) else cam), dtype=np.float64)
        assert cam_h.size >= 4
        info = torch.empty((F - 1, 4), dtype=torch.int32, device=self.device)
        ptr = _lib.ptr
        _lib.call("vus_two_point_ransac", ptr(res.track_idx), ptr(res.kp_keys), ptr(res.kp_count), F, K, self.H, self.W,
                  ptr(rot), cam_h.ctypes.data, thr, int(self.p.ransac_hypotheses), int(self.p.ransac_seed) & 0xFFFFFFFF,
                  ptr(res.track_idx), ptr(info), _lib.current_stream_ptr())
        return info

    def _pair_indices(self, res: FrontendResult, pair_a, pair_b):
        """(a, b) as int32 [n_pairs] device tensors; frame numbers are checked on the host when they come from it."""
        out = []
        for v in (pair_a, pair_b):
            if not isinstance(v, torch.Tensor):
                h = np.asarray(v, dtype=np.int64).reshape(-1)
                assert len(h) >= 1 and (h >= 0).all() and (h < res.n_frames).all(), "pair frame number outside the result"
                v = torch.from_numpy(h.astype(np.int32))
            out.append(v.to(device=self.device, dtype=torch.int32).contiguous())
        assert out[0].shape == out[1].shape and out[0].dim() == 1 and out[0].numel() >= 1
        return out

    def match_keyframes(self, res: FrontendResult, pair_a, pair_b, max_distance: Optional[int] = None,
                        cross_check: bool = True) -> torch.Tensor:
        """Descriptor matches between the LEFT images of arbitrary keyframe pairs (a, b) of `res` -- loop-closure
        candidates, not neighbours: vus_hamming_match on the pairing (2a, 2b) without a geometric gate, Hamming bound
        max_distance (default: track_max_distance), and with cross_check the mutual filter against the swapped
        pairing.  Returns match_idx int32 [n_pairs, K] on the device: left(a) keypoint i -> left(b) keypoint, -1 none."""
        a, b = self._pair_indices(res, pair_a, pair_b)
        n, K, ptr = a.numel(), self.p.max_features, _lib.ptr
        dist = int(self.p.track_max_distance if max_distance is None else max_distance)
        q, t = (2 * a).contiguous(), (2 * b).contiguous()
        idx = torch.empty((n, K), dtype=torch.int32, device=self.device)
        dst = torch.empty((n, K), dtype=torch.int32, device=self.device)
        st = _lib.current_stream_ptr()
        _lib.call("vus_hamming_match", ptr(res.desc), ptr(res.kp_keys), ptr(res.kp_count), K, self.H, self.W, ptr(q), ptr(t), n,
                  -1, 0, 0, dist, ptr(idx), ptr(dst), st)
        if cross_check:
            rev = torch.empty((n, K), dtype=torch.int32, device=self.device)
            _lib.call("vus_hamming_match", ptr(res.desc), ptr(res.kp_keys), ptr(res.kp_count), K, self.H, self.W, ptr(t), ptr(q),
                      n, -1, 0, 0, dist, ptr(rev), ptr(dst), st)
            _lib.call("vus_cross_check", ptr(idx), ptr(rev), n, K, ptr(idx), st)
        return idx

    def keyframe_similarity(self, res: FrontendResult, top: int = 512, max_distance: int = 35, min_gap: int = 0) -> torch.Tensor:
        """Appearance score of every keyframe pair of `res`, from the LEFT images' descriptors alone (vus_keyframe_similarity,
        include/vus_retrieval.h): S[b, a] = how many of keyframe b's first `top` descriptors -- its strongest under the
        global top-K selection; with grid bucketing pass top = max_features -- have a descriptor within max_distance bits
        among keyframe a's first `top`.  Filled for a <= b - min_gap (t_limit[b] = max(b - min_gap + 1, 0)), 0 elsewhere;
        directed: S[b, a] is not S[a, b].  Returns int32 [F, F] on the device.  Asynchronous on the current stream."""
        F, K, ptr = res.n_frames, self.p.max_features, _lib.ptr
        img = (2 * torch.arange(F, dtype=torch.int32, device=self.device)).contiguous()
        limit = (torch.arange(F, dtype=torch.int32, device=self.device) - int(min_gap) + 1).clamp_(min=0).contiguous()
        S = torch.empty((F, F), dtype=torch.int32, device=self.device)
        _lib.call("vus_keyframe_similarity", ptr(res.desc), ptr(res.kp_count), 2 * F, K, ptr(img), F, ptr(img), F, ptr(limit),
                  min(int(top), K), int(max_distance), ptr(S), _lib.current_stream_ptr())   # a front end of fewer slots uses all
        return S

    def relative_poses(self, res: FrontendResult, pair_a, pair_b, match_idx: torch.Tensor, cam5, threshold_px: float = 2.0,
                       n_hyp: int = 256, seed: int = synth.SEED, refine_iters: int = 10,
                       disparity: Optional[torch.Tensor] = None) -> PairPoses:
        """T_a^-1 T_b of every keyframe pair from its matches (match_keyframes) and the stereo matches of both keyframes:
        three-point RANSAC on the triangulated points, then refine_iters Gauss-Newton rounds on the left-image
        reprojection error of the inliers (vus_stereo_pair_pose, include/vus_loop.h; one launch for all pairs).  cam5:
        (fx, fy, cx, cy) in pixels of this H x W image and the baseline in metres.  disparity: refine_stereo()'s disp_q8 --
        the depths then come from the refined disparities (vus_stereo_pair_pose_q8).  Asynchronous on the current stream."""
        if disparity is not None:
            self._check_disparity(res, disparity)
        a, b = self._pair_indices(res, pair_a, pair_b)
        n, K, ptr = a.numel(), self.p.max_features, _lib.ptr
        assert match_idx.dtype == torch.int32 and match_idx.is_cuda and match_idx.is_contiguous() and \
            tuple(match_idx.shape) == (n, K), "match_idx: int32 [n_pairs, K] on the device"
        cam_h = np.ascontiguousarray(cam5.detach().cpu().numpy() if isinstance(cam5, torch.Tensor) else cam5, dtype=np.float64)
        assert cam_h.size == 5, "cam5: fx, fy, cx, cy, baseline"
        dev = self.device
        out = PairPoses(T_ab=torch.empty((n, 12), dtype=torch.float64, device=dev),
                        JtJ=torch.empty((n, 6, 6), dtype=torch.float64, device=dev),
                        rss=torch.empty((n,), dtype=torch.float64, device=dev),
                        info=torch.empty((n, 6), dtype=torch.int32, device=dev),
                        match_idx_out=torch.empty((n, K), dtype=torch.int32, device=dev), pair_a=a, pair_b=b)
        head = (ptr(match_idx), ptr(a), ptr(b), ptr(res.stereo_idx), ptr(res.kp_keys), ptr(res.kp_count), res.n_frames, n, K,
                self.H, self.W, cam_h.ctypes.data, float(threshold_px), int(n_hyp), int(seed) & 0xFFFFFFFF, int(refine_iters))
        tail = (ptr(out.T_ab), ptr(out.JtJ), ptr(out.rss), ptr(out.match_idx_out), ptr(out.info), _lib.current_stream_ptr())
        if disparity is None:
            _lib.call("vus_stereo_pair_pose", *head, *tail)
        else:
            _lib.call("vus_stereo_pair_pose_q8", *head, ptr(disparity), *tail)
        return out

    def refine_relative_poses(self, res: FrontendResult, pair_poses: PairPoses, cam5, sigma_uv_px: float, sigma_disp_px: float,
                              gate: float = 4.0, iters: int = 10, disparity: Optional[torch.Tensor] = None) -> PairBundle:
        """The second stage behind relative_poses() on the pairs of that call (pair_poses.pair_a, pair_b): from its poses and final inliers, `iters` rounds of
        a two-view refit in which the inlier points are free and both stereo observations (x, y, d) of every point enter,
        weighted by sigma_uv_px and sigma_disp_px; a point takes part while its whitened error is at most `gate` sigmas
        (vus_stereo_pair_bundle, include/vus_pair_bundle.h; one launch for all pairs).  A pair relative_poses() gave a
        non-zero status is passed through (status 4).  disparity: the disp_q8 given to relative_poses().  Asynchronous on
        the current stream."""
        if disparity is not None:
            self._check_disparity(res, disparity)
        pp = pair_poses
        assert pp.pair_a is not None and pp.pair_b is not None, "pair_poses: what relative_poses() returned"
        a, b = self._pair_indices(res, pp.pair_a, pp.pair_b)
        n, K, ptr = a.numel(), self.p.max_features, _lib.ptr
        assert tuple(pp.match_idx_out.shape) == (n, K) and tuple(pp.T_ab.shape) == (n, 12) and tuple(pp.info.shape) == (n, 6) \
            and pp.match_idx_out.is_contiguous() and pp.T_ab.is_contiguous() and pp.info.is_contiguous(), \
            "pair_poses: relative_poses() of the same pairs"
        cam_h = np.ascontiguousarray(cam5.detach().cpu().numpy() if isinstance(cam5, torch.Tensor) else cam5, dtype=np.float64)
        assert cam_h.size == 5, "cam5: fx, fy, cx, cy, baseline"
        dev = self.device
        out = PairBundle(T_ab=torch.empty((n, 12), dtype=torch.float64, device=dev),
                         S=torch.empty((n, 6, 6), dtype=torch.float64, device=dev),
                         chi2=torch.empty((n,), dtype=torch.float64, device=dev),
                         points=torch.empty((n, K, 3), dtype=torch.float64, device=dev),
                         info=torch.empty((n, 6), dtype=torch.int32, device=dev),
                         match_idx_out=torch.empty((n, K), dtype=torch.int32, device=dev))
        _lib.call("vus_stereo_pair_bundle", ptr(pp.match_idx_out), ptr(a), ptr(b), ptr(res.stereo_idx), ptr(res.kp_keys),
                  ptr(res.kp_count), res.n_frames, n, K, self.H, self.W, cam_h.ctypes.data,
                  None if disparity is None else ptr(disparity), ptr(pp.T_ab), ptr(pp.info), float(sigma_uv_px),
                  float(sigma_disp_px), float(gate), int(iters), ptr(out.T_ab), ptr(out.S), ptr(out.chi2), ptr(out.points),
                  ptr(out.match_idx_out), ptr(out.info), _lib.current_stream_ptr())
        return out

    def stereo_factors(self, ids: torch.Tensor, feats: torch.Tensor, n_ids: int, Rt: torch.Tensor, cam: torch.Tensor,
                       first_frame: int = 1):
        """What the reference's Python loops make of the CameraMeasurement stream, for all keyframes in two launches
        (vus_emit_stereo_factors): get_landmarks for every feature of every keyframe (batch.py:264-265, 144-176) and
        the landmark loop of batch_create (batch.py:295-305; keyframe 0 has none, hence first_frame = 1).
        ids / feats / n_ids: feature_tracks()'s output; Rt f64 [F,12]: zed_world_transform per keyframe; cam f64 [8]
        as for triangulate().  Returns a dict of device tensors: obs_frame int32 [n], obs_id int64 [n],
        obs_meas f64 [n,3] (uL, uR, v) in batch_create's factor order; lm_first int64 [n_ids] (-1: id not seen in
        keyframes >= first_frame), lm_point f64 [n_ids,3] (first-sighting world point = initial value of L(id))."""
        F, K = ids.shape
        dev = ids.device
        assert Rt.shape == (F, 12) and Rt.dtype == torch.float64 and Rt.is_contiguous() and cam.numel() == 8
        cap = F * K
        base = torch.empty((F + 1,), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        of = torch.empty((cap,), dtype=torch.int32, device=dev)
        oi = torch.empty((cap,), dtype=torch.int64, device=dev)
        om = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        first = torch.empty((max(n_ids, 1),), dtype=torch.int64, device=dev)
        pt = torch.zeros((max(n_ids, 1), 3), dtype=torch.float64, device=dev)
        ptr = _lib.ptr
        _lib.call("vus_emit_stereo_factors", ptr(ids), ptr(feats), ptr(Rt), ptr(cam), F, K, int(first_frame), int(n_ids),
                  ptr(base), ptr(count), ptr(of), ptr(oi), ptr(om), ptr(first), ptr(pt), _lib.current_stream_ptr())
        n = int(count.item())
        return {"obs_frame": of[:n], "obs_id": oi[:n], "obs_meas": om[:n], "lm_first": first[:n_ids],
                "lm_point": pt[:n_ids]}

    def camera_measurements(self, res: FrontendResult, disparity: Optional[torch.Tensor] = None) -> List[CameraMeasurement]:
        """Per frame, the published features as CameraMeasurement records (message shape of
        batch.py:149-154), built from feature_tracks(); disparity as there."""
        ids, feats, _ = self.feature_tracks(res, disparity)
        ids, feats = ids.cpu().numpy(), feats.cpu().numpy()
        out = []
        for f in range(res.n_frames):
            msg = CameraMeasurement()
            for i in (ids[f] >= 0).nonzero()[0].tolist():
                u0, v0, u1, v1 = feats[f, i]
                msg.features.append(Feature(id=int(ids[f, i]), u0=float(u0), v0=float(v0), u1=float(u1), v1=float(v1)))
            out.append(msg)
        return out


def triangulate(feat: torch.Tensor, cam: torch.Tensor, Rt: torch.Tensor) -> torch.Tensor:
    """get_landmarks (batch.py:144-176) on the GPU: feat [n,4] f64 (u0,v0,u1,v1), cam [8] f64
    (fx,fy,cx,cy,baseline,res_x,res_y,0), Rt [12] f64 -> [n,6] (X,Y,Z,uL,uR,v)."""
    _lib.require_gpu()
    assert feat.dtype == torch.float64 and feat.is_cuda and feat.is_contiguous() and feat.shape[1] == 4
    out = torch.empty((feat.shape[0], 6), dtype=torch.float64, device=feat.device)
    _lib.call("vus_triangulate", _lib.ptr(feat), feat.shape[0], _lib.ptr(cam), _lib.ptr(Rt), _lib.ptr(out),
              _lib.current_stream_ptr())
    return out
