"""The numpy statement of lens undistortion + stereo rectification (include/vus_rectify.h): camera models,
rectifying rotations, the Q5 map, the per-tile plan and the remap -- written independently of
visual_underwater_slam_amd/rectify.py (which imports nothing from here) -- plus the test rig and its raw render.

Test infrastructure only."""
import numpy as np

from visual_underwater_slam_amd import synth
from visual_underwater_slam_amd.frontend import default_camera

TILE_W, TILE_H, LDS_BYTES = 64, 16, 8192

# ---------------------------------------------------------------------------------------------------------------------
# models


def distort(model, k, xn, yn):
    xn, yn = np.asarray(xn, np.float64), np.asarray(yn, np.float64)
    if model == "none":
        return xn.copy(), yn.copy()
    if model == "radtan":
        k1, k2, p1, p2 = k[:4]
        k3 = k[4] if len(k) == 5 else 0.0
        rr = xn ** 2 + yn ** 2
        g = 1.0 + k1 * rr + k2 * rr ** 2 + k3 * rr ** 3
        xy = xn * yn
        return g * xn + (2.0 * p1 * xy + p2 * (rr + 2.0 * xn ** 2)), g * yn + (p1 * (rr + 2.0 * yn ** 2) + 2.0 * p2 * xy)
    assert model == "equidistant"
    r = np.hypot(xn, yn)
    th = np.arctan(r)
    thd = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 1e-12, thd / r, 1.0)
    return s * xn, s * yn


def undistort(model, k, xd, yd, rounds=30):
    x, y = np.array(xd, np.float64), np.array(yd, np.float64)
    for _ in range(rounds):
        ex, ey = distort(model, k, x, y)
        x, y = x - (ex - xd), y - (ey - yd)
    return x, y


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-15:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def rotations(T10):
    """R0, R1, baseline by Gram-Schmidt on (baseline direction, mean optical axis)."""
    R10, t10 = T10[:3, :3], T10[:3, 3]
    c = -(R10.T @ t10)
    b = np.sqrt(c @ c)
    ex = c / b
    axis = R10.T[:, 2] + np.array([0.0, 0.0, 1.0])
    ez = axis - (axis @ ex) * ex
    ez /= np.sqrt(ez @ ez)
    ey = np.cross(ez, ex)
    R0 = np.array([ex, ey, ez])
    return R0, R0 @ R10.T, b


def source_uv(new_cam, R, K_raw, model, k, H, W):
    """Real source coordinates (u, v) [H, W] of every rectified pixel: rays as 3-vectors, rotated back by R^T."""
    fx, fy, cx, cy = new_cam
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)
    p = rays @ R          # row vector times R = R^T times column vector
    xd, yd = distort(model, k, p[..., 0] / p[..., 2], p[..., 1] / p[..., 2])
    return K_raw[0] * xd + K_raw[2], K_raw[1] * yd + K_raw[3]


def q5_words(u, v):
    H, W = u.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    dx = np.floor((u - xs) * 32 + 0.5).astype(np.int64)
    dy = np.floor((v - ys) * 32 + 0.5).astype(np.int64)
    assert dx.min() >= -32768 and dx.max() <= 32767 and dy.min() >= -32768 and dy.max() <= 32767
    return pack_words(dx, dy)


def pack_words(dx, dy):
    return ((np.asarray(dy, np.int64) << 16) | (np.asarray(dx, np.int64) & 0xFFFF)).astype(np.uint32).view(np.int32)


def unpack_words(words):
    w = np.asarray(words, np.int32).astype(np.int64)
    dx = ((w & 0xFFFF) ^ 0x8000) - 0x8000
    return dx, w >> 16


# ---------------------------------------------------------------------------------------------------------------------
# remap and plan (integers)


def taps(words):
    """x0, x1, y0, y1, fx, fy [H, W] of one map."""
    H, W = words.shape
    dx, dy = unpack_words(words)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    sx, sy = (xs << 5) + dx, (ys << 5) + dy
    ix, iy = sx >> 5, sy >> 5
    return (np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1),
            sx & 31, sy & 31)


def remap(src, maps):
    """src uint8 [n, H, W], maps int32 [n_maps, H, W] -> uint8 [n, H, W]; image i uses map i % n_maps."""
    src = np.asarray(src)
    out = np.empty_like(src)
    tp = [taps(m) for m in maps]
    for i in range(len(src)):
        x0, x1, y0, y1, fx, fy = tp[i % len(maps)]
        s = src[i].astype(np.int64)
        acc = (s[y0, x0] * (32 - fx) * (32 - fy) + s[y0, x1] * fx * (32 - fy) + s[y1, x0] * (32 - fx) * fy
               + s[y1, x1] * fx * fy + 512)
        out[i] = (acc >> 10).astype(np.uint8)
    return out


def plan(maps):
    """int32 [n_maps, tiles_y, tiles_x, 4] source boxes (x0, y0, w, h); all zero where the box is over the LDS budget."""
    n, H, W = maps.shape
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    boxes = np.zeros((n, ty, tx, 4), np.int32)
    for m in range(n):
        x0, x1, y0, y1, _, _ = taps(maps[m])
        for j in range(ty):
            for i in range(tx):
                sl = (slice(j * TILE_H, (j + 1) * TILE_H), slice(i * TILE_W, (i + 1) * TILE_W))
                bx, by = x0[sl].min(), y0[sl].min()
                w, h = x1[sl].max() - bx + 1, y1[sl].max() - by + 1
                if ((w + 6) & ~3) * h <= LDS_BYTES:
                    boxes[m, j, i] = (bx, by, w, h)
    return boxes


def plan_brute(maps):
    """The same boxes pixel by pixel, from the REMAP statement alone."""
    n, H, W = maps.shape
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    lo = np.full((n, ty, tx, 2), 1 << 30, np.int64)
    hi = np.full((n, ty, tx, 2), -1, np.int64)
    for m in range(n):
        for y in range(H):
            for x in range(W):
                w = int(maps[m, y, x])
                dx, dy = ((w & 0xFFFF) ^ 0x8000) - 0x8000, w >> 16
                ix, iy = ((x << 5) + dx) >> 5, ((y << 5) + dy) >> 5
                xs = (min(max(ix, 0), W - 1), min(max(ix + 1, 0), W - 1))
                ys = (min(max(iy, 0), H - 1), min(max(iy + 1, 0), H - 1))
                t = (m, y // TILE_H, x // TILE_W)
                lo[t] = np.minimum(lo[t], (min(xs), min(ys)))
                hi[t] = np.maximum(hi[t], (max(xs), max(ys)))
    wh = hi - lo + 1
    boxes = np.concatenate([lo, wh], -1)
    fits = ((wh[..., 0] + 6) & ~3) * wh[..., 1] <= LDS_BYTES
    return np.where(fits[..., None], boxes, 0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# synthetic maps of the kernel tests


def identity_map(H, W):
    return np.zeros((H, W), np.int32)


def shift_map(H, W, q5x, q5y):
    return pack_words(np.full((H, W), q5x), np.full((H, W), q5y))


def rotate180_map(H, W):
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    return pack_words(((W - 1 - xs) - xs) * 32, ((H - 1 - ys) - ys) * 32)


def shrink_map(H, W, factor=5):
    """Output pixel (x, y) looks at factor * (x, y) about the image centre: a tile's footprint is factor times the tile."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    cx, cy = (W - 1) // 2, (H - 1) // 2
    return pack_words((factor - 1) * (xs - cx) * 32 + 7, (factor - 1) * (ys - cy) * 32 + 19)


def random_map(H, W, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, (H, W), dtype=np.int64).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the test rig

RIG_SCALE0, RIG_SCALE1 = (1.01, 1.012, 0.99, 1.02), (0.995, 0.99, 1.015, 0.985)
RIG_ROT = (0.01, -0.015, 0.008)
RIG_T = (-0.063, 0.0008, -0.0012)
RIG_DIST = {"radtan": ((-0.28, 0.09, 4e-4, -3e-4, -0.012), (-0.27, 0.085, -2e-4, 5e-4, -0.01)),
            "equidistant": ((-0.03, 0.01, -0.004, 0.001), (-0.028, 0.012, -0.003, 0.0008))}


class Rig:
    """Raw intrinsics, distortion and extrinsics of the test rig at H x W; new camera = default_camera(H, W)."""

    def __init__(self, model, H, W):
        self.model, self.H, self.W = model, H, W
        self.new_cam = default_camera(H, W)
        self.K = (self.new_cam * np.array(RIG_SCALE0), self.new_cam * np.array(RIG_SCALE1))
        self.dist = tuple(np.array(d) for d in RIG_DIST[model])
        R10 = exp_so3(RIG_ROT)
        t10 = np.array(RIG_T)
        t10 = t10 / np.linalg.norm(R10.T @ t10) * synth.BASELINE_M
        self.T10 = np.eye(4)
        self.T10[:3, :3], self.T10[:3, 3] = R10, t10
        self.R0, self.R1, self.baseline = rotations(self.T10)

    def maps(self, new_cam=None):
        cam = self.new_cam if new_cam is None else new_cam
        return np.stack([q5_words(*source_uv(cam, R, self.K[c], self.model, self.dist[c], self.H, self.W))
                         for c, R in enumerate((self.R0, self.R1))])

    def kalibr(self):
        """The rig as a Kalibr camchain dict (plain lists, as YAML gives them)."""
        out = {}
        for c in (0, 1):
            out[f"cam{c}"] = dict(camera_model="pinhole", intrinsics=[float(v) for v in self.K[c]],
                                  distortion_model=self.model, distortion_coeffs=[float(v) for v in self.dist[c]],
                                  resolution=[self.W, self.H])
        out["cam1"]["T_cn_cnm1"] = [[float(v) for v in row] for row in self.T10]
        return out

    def rays(self, c, xp=np, device=None):
        """Unit-depth rays [H, W] x 3 of raw camera c's pixels in the RECTIFIED frame (numpy float64 or torch on device)."""
        K, R = self.K[c], (self.R0, self.R1)[c]
        xs, ys = np.meshgrid(np.arange(self.W, dtype=np.float64), np.arange(self.H, dtype=np.float64))
        xn, yn = undistort(self.model, self.dist[c], (xs - K[2]) / K[0], (ys - K[3]) / K[1])
        a = R[0, 0] * xn + R[0, 1] * yn + R[0, 2]
        b = R[1, 0] * xn + R[1, 1] * yn + R[1, 2]
        d = R[2, 0] * xn + R[2, 1] * yn + R[2, 2]
        if xp is np:
            return a, b, d
        return tuple(xp.from_numpy(v).to(device) for v in (a, b, d))


def render_raw_view(rays, T12, c, t, H, W, xp=np, device=None, seed=synth.SEED):
    """synth.render_plane_view's ray cast for a RAW camera: `rays` from Rig.rays (rectified frame, which is the frame of
    pose T12), camera centre displaced by c * BASELINE_M along the rectified x axis; the same texture and noise hashes."""
    a, b, d = rays
    R = [float(v) for v in T12[:9]]
    o = [float(T12[9 + r]) + R[3 * r] * synth.BASELINE_M * c for r in range(3)]
    dz = (a * R[6] + b * R[7]) + d * R[8]
    lam = (synth.SCENE_PLANE_Z - o[2]) / dz
    px = ((a * R[0] + b * R[1]) + d * R[2]) * lam + o[0]
    py = ((a * R[3] + b * R[4]) + d * R[5]) * lam + o[1]
    if xp is np:
        bx = np.floor(px / synth.SCENE_TEXEL).astype(np.int64) + 32768
        by = np.floor(py / synth.SCENE_TEXEL).astype(np.int64) + 32768
    else:
        bx = xp.floor(px / synth.SCENE_TEXEL).to(xp.int64) + 32768
        by = xp.floor(py / synth.SCENE_TEXEL).to(xp.int64) + 32768
    base = synth._mix32((((bx & 0xFFFF) << 16) | (by & 0xFFFF)) ^ synth._mix32_scalar(seed ^ 0x5CE7E)) & 255
    pix = synth._arange(xp, H, device)[:, None] * W + synth._arange(xp, W, device)[None, :]
    k = synth._mix32_scalar(synth._mix32_scalar((seed + t) & synth._M) ^ (0x9E3779B9 * (c + 1)))
    img = base + (synth._mix32(pix ^ k) % 9 - 4)
    img = img.clip(0, 255) if xp is np else img.clamp(0, 255)
    return img.astype(np.uint8) if xp is np else img.to(xp.uint8)


def raw_frames(rig, poses, xp=np, device=None):
    """Raw stereo pairs uint8 [n, 2, H, W] of synth's textured plane from the rectified-left-camera poses [n, 12]."""
    rays = [rig.rays(c, xp, device) for c in (0, 1)]
    out = []
    for t in range(len(poses)):
        pair = [render_raw_view(rays[c], poses[t], c, t, rig.H, rig.W, xp, device) for c in (0, 1)]
        out.append(np.stack(pair) if xp is np else xp.stack(pair))
    return np.stack(out) if xp is np else xp.stack(out)
