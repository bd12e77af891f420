"""Raw camera input: lens undistortion and stereo rectification in front of `StereoOrbFrontend.process`.

The reference's launch file hands its image-processor nodelet the RAW camera topics together with a Kalibr / msckf-style
calibration file (distortion model, coefficients, `T_cn_cnm1`; launch/stereo.launch:5-6, 15, 23-25).  The front end here
takes ideal, row-aligned pinhole images, so a raw stream passes through `StereoRectifier.rectify` first: one
`vus_rectify_remap` launch (include/vus_rectify.h) over the whole resident batch.

The host part -- camera models, the rectifying rotations, the zoom that keeps every rectified pixel inside its raw image,
and the Q5 remap table -- is plain numpy float64: it runs once per calibration.  The table's per-tile source boxes
(`vus_rectify_plan`) and the remap itself run on the GPU; there is no CPU fallback.
"""
from typing import Sequence

import numpy as np

MODELS = ("radtan", "equidistant", "none")
UNDISTORT_ROUNDS = 30
ZOOM_RANGE = (0.25, 4.0)
ZOOM_STEPS = 40
Q5 = 32


class CameraModel:
    """Pinhole intrinsics (fx, fy, cx, cy) and a lens distortion in Kalibr's terms: "radtan" (k1, k2, p1, p2[, k3], the
    plumb-bob form), "equidistant" (k1..k4 on theta = atan r) or "none".  All methods are elementwise on numpy arrays of
    normalised image coordinates."""

    def __init__(self, intrinsics: Sequence[float], distortion_model: str = "none", distortion_coeffs: Sequence[float] = ()):
        if distortion_model not in MODELS:
            raise ValueError(f"distortion_model {distortion_model!r}: expected one of {MODELS}")
        self.intrinsics = np.asarray(intrinsics, dtype=np.float64).reshape(-1)
        if self.intrinsics.shape != (4,) or not (self.intrinsics[:2] > 0).all():
            raise ValueError("intrinsics: expected (fx, fy, cx, cy) with positive focal lengths")
        d = np.asarray(distortion_coeffs, dtype=np.float64).reshape(-1)
        want = {"radtan": (4, 5), "equidistant": (4,), "none": (0, 4, 5)}[distortion_model]
        if len(d) not in want:
            raise ValueError(f"{distortion_model}: {len(d)} distortion coefficients, expected {' or '.join(map(str, want))}")
        self.distortion_model = distortion_model
        self.distortion_coeffs = d

    def distort(self, xn, yn):
        xn, yn = np.asarray(xn, dtype=np.float64), np.asarray(yn, dtype=np.float64)
        if self.distortion_model == "none":
            return xn + 0.0 * yn, yn + 0.0 * xn
        d = self.distortion_coeffs
        if self.distortion_model == "radtan":
            k1, k2, p1, p2 = d[:4]
            k3 = d[4] if len(d) > 4 else 0.0
            r2 = xn * xn + yn * yn
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            return (xn * radial + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn),
                    yn * radial + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn)
        k1, k2, k3, k4 = d
        r = np.sqrt(xn * xn + yn * yn)
        th = np.arctan(r)
        t2 = th * th
        thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(r > 1e-12, thd / np.maximum(r, 1e-300), 1.0)
        return xn * s, yn * s

    def undistort(self, xd, yd):
        """The inverse of distort by fixed-point iteration, x <- x + (xd - distort(x)), UNDISTORT_ROUNDS rounds."""
        xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
        x, y = xd + 0.0 * yd, yd + 0.0 * xd
        if self.distortion_model == "none":
            return x, y
        for _ in range(UNDISTORT_ROUNDS):
            ex, ey = self.distort(x, y)
            x, y = x + (xd - ex), y + (yd - ey)
        return x, y

    def project(self, points):
        """Pixel coordinates [..., 2] of points [..., 3] in the camera frame."""
        p = np.asarray(points, dtype=np.float64)
        xd, yd = self.distort(p[..., 0] / p[..., 2], p[..., 1] / p[..., 2])
        fx, fy, cx, cy = self.intrinsics
        return np.stack([fx * xd + cx, fy * yd + cy], axis=-1)


def rectifying_rotations(T_cn_cnm1):
    """(R0, R1, baseline) from the 4 x 4 transform that takes cam0 coordinates to cam1 coordinates (Kalibr's T_cn_cnm1).
    R_c takes camera c's coordinates to the rectified frame: x along the baseline from cam0 to cam1, z the mean optical
    axis made orthogonal to it.  A point's rectified cam1 coordinates are its rectified cam0 coordinates minus
    (baseline, 0, 0)."""
    T = np.asarray(T_cn_cnm1, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("T_cn_cnm1: expected a 4 x 4 matrix")
    R10, t10 = T[:3, :3], T[:3, 3]
    c = -R10.T @ t10                               # cam1's centre in cam0
    baseline = float(np.linalg.norm(c))
    if not baseline > 0.0:
        raise ValueError("T_cn_cnm1: the two cameras share a centre")
    e_x = c / baseline
    z = np.array([0.0, 0.0, 1.0]) + R10.T @ np.array([0.0, 0.0, 1.0])
    e_z = z - e_x * (e_x @ z)
    e_z = e_z / np.linalg.norm(e_z)
    e_y = np.cross(e_z, e_x)
    R0 = np.stack([e_x, e_y, e_z])
    return R0, R0 @ R10.T, baseline


def source_coordinates(new_camera, R, cam: CameraModel, H: int, W: int, xs=None, ys=None):
    """(u, v) float64 [H, W]: where rectified pixel (x, y) of the camera with rectifying rotation R lies in its raw image.
    With xs, ys (arrays of one shape): the same for those pixels only."""
    fx, fy, cx, cy = (float(v) for v in new_camera)
    if xs is None:
        xs, ys = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    xr = (np.asarray(xs, dtype=np.float64) - cx) / fx
    yr = (np.asarray(ys, dtype=np.float64) - cy) / fy
    Rt = np.asarray(R, dtype=np.float64).T
    X = Rt[0, 0] * xr + Rt[0, 1] * yr + Rt[0, 2]
    Y = Rt[1, 0] * xr + Rt[1, 1] * yr + Rt[1, 2]
    Z = Rt[2, 0] * xr + Rt[2, 1] * yr + Rt[2, 2]
    xd, yd = cam.distort(X / Z, Y / Z)
    kx, ky, ku, kv = cam.intrinsics
    return kx * xd + ku, ky * yd + kv


def quantise_map(u, v) -> np.ndarray:
    """int32 [H, W] map words (dy << 16) | (dx & 0xFFFF) of include/vus_rectify.h from real source coordinates."""
    H, W = u.shape
    dx = np.floor((u - np.arange(W, dtype=np.float64)[None, :]) * Q5 + 0.5)
    dy = np.floor((v - np.arange(H, dtype=np.float64)[:, None]) * Q5 + 0.5)
    for name, d in (("x", dx), ("y", dy)):
        if not np.isfinite(d).all():
            raise ValueError(f"the {name} displacement of the model is not finite: it cannot enter the int16 Q5 map")
        if d.min() < -32768 or d.max() > 32767:
            raise ValueError(f"the {name} displacement of the model leaves the int16 range of the Q5 map "
                             f"(+-1024 pixels): {d.min() / Q5:.0f} .. {d.max() / Q5:.0f} pixels")
    word = (dy.astype(np.int64) << 16) | (dx.astype(np.int64) & 0xFFFF)
    return word.astype(np.int32)


def fit_zoom(cams, rotations, focal: float, H: int, W: int) -> float:
    """The smallest zoom z in ZOOM_RANGE (bisection, ZOOM_STEPS steps) at which every pixel of the outer frame of both
    rectified images, seen through (z focal, z focal, (W-1)/2, (H-1)/2), maps inside its raw image."""
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    xs = np.concatenate([x, x, 0 * y, 0 * y + (W - 1)])
    ys = np.concatenate([0 * x, 0 * x + (H - 1), y, y])

    def inside(z):
        for cam, R in zip(cams, rotations):
            u, v = source_coordinates((z * focal, z * focal, (W - 1) / 2.0, (H - 1) / 2.0), R, cam, H, W, xs, ys)
            if not ((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)).all():   # NaN counts as outside
                return False
        return True

    lo, hi = ZOOM_RANGE
    if not inside(hi):
        raise ValueError(f"no zoom up to {hi} keeps the rectified images inside the raw images: check the calibration")
    if inside(lo):
        return lo
    for _ in range(ZOOM_STEPS):
        mid = 0.5 * (lo + hi)
        if inside(mid):
            hi = mid
        else:
            lo = mid
    return hi


class StereoRectifier:
    """Rectifies raw stereo pairs of one calibration.

    cam0, cam1: CameraModel of the raw left / right camera; T_cn_cnm1: cam0 -> cam1 coordinates (4 x 4); size = (H, W)
    of raw AND rectified images.  new_camera = (fx, fy, cx, cy) of both rectified images, taken as given (source
    positions outside the raw image replicate its border); None fits it: fx = fy = z * mean of the four raw focal
    lengths, principal point at the image centre, z from fit_zoom.

    Members: maps int32 [2, H, W] and boxes int32 [2, tiles_y, tiles_x, 4] on the device (include/vus_rectify.h; made
    on first use, maps_host is the numpy table), camera (fx, fy, cx, cy), baseline, R0, R1 (raw camera -> rectified
    frame)."""

    def __init__(self, cam0: CameraModel, cam1: CameraModel, T_cn_cnm1, size, new_camera=None, device: str = "cuda:0"):
        self.H, self.W = int(size[0]), int(size[1])
        self.cam0, self.cam1 = cam0, cam1
        self.R0, self.R1, self.baseline = rectifying_rotations(T_cn_cnm1)
        H, W = self.H, self.W
        if new_camera is None:
            focal = float(np.mean([cam0.intrinsics[0], cam0.intrinsics[1], cam1.intrinsics[0], cam1.intrinsics[1]]))
            self.zoom = fit_zoom((cam0, cam1), (self.R0, self.R1), focal, H, W)
            self.camera = np.array([self.zoom * focal, self.zoom * focal, (W - 1) / 2.0, (H - 1) / 2.0])
        else:
            self.zoom = None
            self.camera = np.asarray(new_camera, dtype=np.float64).reshape(4).copy()
        self.maps_host = np.stack([quantise_map(*source_coordinates(self.camera, R, cam, H, W))
                                   for cam, R in ((cam0, self.R0), (cam1, self.R1))])
        self.device = device
        self._maps = self._boxes = self._out = None

    def _upload(self):
        """The device side, on first use: the host part above needs no GPU."""
        import torch
        from . import _abi, _lib
        _lib.require_gpu()
        self.device = torch.device(self.device)
        self._maps = torch.from_numpy(self.maps_host).to(self.device)
        tiles_y = -(-self.H // _abi.const("VUS_RECTIFY_TILE_H"))
        tiles_x = -(-self.W // _abi.const("VUS_RECTIFY_TILE_W"))
        self._boxes = torch.empty((2, tiles_y, tiles_x, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("vus_rectify_plan", _lib.ptr(self._maps), 2, self.H, self.W, _lib.ptr(self._boxes),
                      _lib.current_stream_ptr())

    @property
    def maps(self):
        if self._maps is None:
            self._upload()
        return self._maps

    @property
    def boxes(self):
        if self._boxes is None:
            self._upload()
        return self._boxes

    @classmethod
    def from_kalibr(cls, d_or_path, size, new_camera=None, device: str = "cuda:0"):
        """From a Kalibr camchain: a dict, or the path of its YAML file, with cam0 / cam1 holding intrinsics,
        distortion_model, distortion_coeffs, resolution ([W, H]) and, in cam1, T_cn_cnm1."""
        if isinstance(d_or_path, dict):
            d = d_or_path
        else:
            import yaml
            with open(d_or_path) as f:
                d = yaml.safe_load(f)
        H, W = int(size[0]), int(size[1])
        cams = []
        for name in ("cam0", "cam1"):
            c = d[name]
            if "resolution" in c and [int(v) for v in c["resolution"]] != [W, H]:
                raise ValueError(f"{name}: calibrated at resolution {list(c['resolution'])} (W, H), images are {[W, H]}: "
                                 f"a raw size different from the rectified size is not supported")
            cams.append(CameraModel(c["intrinsics"], c.get("distortion_model", "none"), c.get("distortion_coeffs", ())))
        return cls(cams[0], cams[1], np.asarray(d["cam1"]["T_cn_cnm1"], dtype=np.float64), (H, W), new_camera, device)

    def rectify(self, raw, out=None):
        """raw uint8 [F, 2, H, W] on the device (index 1: 0 = cam0, 1 = cam1) -> rectified uint8 [F, 2, H, W]: one
        vus_rectify_remap launch on the current stream.  Without `out` the result lives in a buffer of this object that
        the next call of the same F reuses."""
        import torch
        from . import _lib
        assert raw.dtype == torch.uint8 and raw.is_cuda and raw.is_contiguous()
        assert raw.dim() == 4 and tuple(raw.shape[1:]) == (2, self.H, self.W), "raw: expected uint8 [F, 2, H, W]"
        if out is None:
            if self._out is None or self._out.shape != raw.shape or self._out.device != raw.device:
                self._out = torch.empty_like(raw)
            out = self._out
        assert out.dtype == torch.uint8 and out.shape == raw.shape and out.is_contiguous() and out.device == raw.device
        assert out.data_ptr() != raw.data_ptr(), "rectify cannot work in place"
        _lib.call("vus_rectify_remap", _lib.ptr(raw), 2 * raw.shape[0], self.H, self.W, self.W, _lib.ptr(self.maps),
                  _lib.ptr(self.boxes), 2, _lib.ptr(out), self.W, _lib.current_stream_ptr())
        return out

    # -- what the stages after the front end take -------------------------------------------------------------------
    def cal3_s2_stereo(self):
        from . import gtsam
        fx, fy, cx, cy = self.camera
        return gtsam.Cal3_S2Stereo(fx, fy, 0.0, cx, cy, self.baseline)

    def cam_array(self, disparity_sign: int = 1):
        """(fx, fy, cx, cy, baseline, W, H, 0) on the device, as `triangulate` and `stereo_factors` take it: the camera is
        given in pixels of the H x W image, so the resolution entries are W and H.  disparity_sign = +1 enters as a
        negated baseline, as in BatchSequence.cam_array."""
        import torch
        assert disparity_sign in (-1, 1)
        b = self.baseline if disparity_sign < 0 else -self.baseline
        return torch.tensor([*self.camera, b, float(self.W), float(self.H), 0.0], dtype=torch.float64, device=self.maps.device)

    def sensor_pose(self, body_P_cam0=None):
        """body_P_sensor of the rectified left camera: body_P_cam0 o Pose3(R0^T, 0)."""
        from . import gtsam
        rect = gtsam.Pose3(gtsam.Rot3(self.R0.T), np.zeros(3))
        return rect if body_P_cam0 is None else gtsam.Pose3(body_P_cam0).compose(rect)
