"""The reference's batch path end to end: stereo images -> front-end -> CameraMeasurement features -> get_landmarks
-> batch_update / batch_create -> LevenbergMarquardtOptimizer.optimize().

Host mirror of the parts of `AUV_ISAM` (/root/reference/batch.py) that lie on that path -- constants of batch.py:88-118,
`get_landmarks` (:144-176), `batch_update` (:253-266), `batch_create` (:270-305) and the optimiser call (:337) -- with
the ROS transport (subscribers, TF listener, time synchroniser; SURVEY.md out of scope) replaced by plain arguments.

Two ways from the front-end's output to the factor graph, producing the SAME graph:
  * `batch_update()` + `batch_create()`: the reference's own per-message / per-landmark Python loops, through the
    gtsam-shaped API (one GenericStereoFactor3D object per observation) -- what batch.py does, unchanged;
  * `batch_create_from_tracks()`: the whole stream at once -- `StereoOrbFrontend.stereo_factors` (vus_emit_stereo_factors)
    turns (ids, features, keyframe transforms) into factor arrays on the GPU, which enter the graph as ONE
    StereoFactorBlock and ONE insert_point3_block (first-sighting initialisation, keyframe 0 skipped, like the loop).

Two documented deviations from the reference's text, both switchable:
  * DVL factor: `gtsam.DvlVelocityFactor` (correct Jacobians) instead of the CustomFactor of batch.py:196-250, whose
    Jacobians are ill-formed.
  * `disparity_sign`: batch.py:156 computes `d = uR - uL`.  For a rig whose cam0 is the left camera that is negative, the
    triangulated point lands BEHIND the camera (z_cam = f * baseline / d < 0), every stereo factor then takes gtsam's
    cheirality branch (constant residual, zero Jacobians) and the landmarks never move.  `disparity_sign=-1` (default)
    is the reference verbatim; `disparity_sign=+1` evaluates the same formulas with the baseline's sign flipped
    (d / (-baseline) = (uL - uR) / baseline), which is the geometrically valid triangulation.  Both run the same kernel.
"""
from dataclasses import InitVar, dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import gtsam
from . import synth
from .frontend import CameraMeasurement, ImageProcessorParams, StereoOrbFrontend, default_camera, triangulate
from .gtsam.symbol_shorthand import B, L, V, X


def vector3(x, y, z):
    return np.array([x, y, z], dtype=float)


def depth_from_pressure(press_abs):
    """process_depth (batch.py:122-126): absolute pressure in hPa -> the depth that replaces the odometry's z
    (process_odom, batch.py:133-134).  Pinned by tests/golden/ref_batch_*.npz (the reference's own output)."""
    measured_pressure = press_abs * 100
    pressure_diff = measured_pressure - 98250.0
    return pressure_diff / (997 * 9.81)


class BatchSequence:
    """AUV_ISAM's batch accumulators and graph construction (batch.py:74-118, 144-176, 253-305)."""

    def __init__(self, disparity_sign: int = -1, device: str = "cuda:0", body_P_sensor: Optional["gtsam.Pose3"] = None):
        """body_P_sensor: the camera-to-body extrinsic put on every stereo factor (the reference builds it as DELTA,
        batch.py:190-193, and never passes it on); X(i) is then the body pose.  Landmarks are initialised from
        zed_world_transform -- the CAMERA in the world -- as in the reference (batch.py:166)."""
        assert disparity_sign in (-1, 1)
        self.body_P_sensor = None if body_P_sensor is None else gtsam.Pose3(body_P_sensor)
        self.device = torch.device(device)
        self.graph = gtsam.NonlinearFactorGraph()                                    # batch.py:80
        self.initial_estimate = gtsam.Values()                                       # :81
        self.timestep = 0
        # IMU (:87-92, 178-193)
        self.grav = 9.81
        self.g = np.array([0, 0, -self.grav])
        self.PARAMS = gtsam.PreintegrationParams.MakeSharedU(self.grav)
        I = np.eye(3)
        self.PARAMS.setAccelerometerCovariance(I * 8.999999999999999e-08)
        self.PARAMS.setGyroscopeCovariance(I * 1.2184696791468346e-07)
        self.PARAMS.setIntegrationCovariance(I * 1e-07)
        self.imu_preintegrated = gtsam.PreintegratedImuMeasurements(self.PARAMS)
        self.prev_bias = gtsam.imuBias.ConstantBias()
        # noise models (:95-98)
        self.pose_noise = gtsam.noiseModel.Diagonal.Sigmas(np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))
        self.vel_noise = gtsam.noiseModel.Isotropic.Sigma(3, 0.1)
        self.dvl_noise = gtsam.noiseModel.Isotropic.Sigma(3, 0.1)
        # accumulators (:99-108)
        self.imu_data: List[np.ndarray] = []
        self.odom_accum, self.dvl_accum, self.imu_accum, self.landmark_accum = [], [], [], []
        self.zed_world_transform = None
        # camera (:110-118)
        self.baseline = 0.063
        self.intrinsic = [1827.0, 1827.5999755859375, 968.9000244140625, 561.4000244140625]
        self.f = (self.intrinsic[0] + self.intrinsic[1]) / 2.0
        self.cx, self.cy = self.intrinsic[2], self.intrinsic[3]
        self.K = gtsam.Cal3_S2Stereo(self.intrinsic[0], self.intrinsic[1], 0.0, self.cx, self.cy, self.baseline)
        self.resolution_x, self.resolution_y = 1920, 1080
        self.landmark_noise = gtsam.noiseModel.Isotropic.Sigma(3, 10)
        self.disparity_sign = disparity_sign
        self._tf_accum = []

    # -- camera ---------------------------------------------------------------------------------------------------
    def cam_array(self) -> torch.Tensor:
        """(fx, fy, cx, cy, baseline, resolution_x, resolution_y, 0) for vus_triangulate.  The reference's
        `d = uR - uL` (batch.py:156) is kept in the kernel; disparity_sign=+1 enters as a negated baseline."""
        b = self.baseline if self.disparity_sign < 0 else -self.baseline
        return torch.tensor([*self.intrinsic, b, self.resolution_x, self.resolution_y, 0.0], dtype=torch.float64,
                            device=self.device)

    def set_zed_world_transform(self, rot, trans):
        """What the TF callback stores (batch.py:45-48): (Rot3, translation)."""
        self.zed_world_transform = (rot, np.asarray(trans, dtype=float).reshape(3))

    def update_imu(self, acc, gyro):                                                 # batch.py:138-141
        self.imu_data.append(np.hstack((np.asarray(acc, float), np.asarray(gyro, float))))

    # -- batch.py:144-176 -----------------------------------------------------------------------------------------
    def get_landmarks(self, data: CameraMeasurement):
        landmarks = []
        if self.zed_world_transform is not None and len(data.features):              # :148
            feat = torch.tensor([[f.u0, f.v0, f.u1, f.v1] for f in data.features], dtype=torch.float64, device=self.device)
            Rt = torch.from_numpy(np.concatenate([self.zed_world_transform[0].matrix().reshape(-1),
                                                  self.zed_world_transform[1]])).to(self.device)
            out = triangulate(feat, self.cam_array(), Rt).cpu().numpy()              # :152-166 on the GPU
            for f, o in zip(data.features, out):
                landmarks.append({'id': f.id, 'pose': o[:3].copy(), 'uL': float(o[3]), 'uR': float(o[4]), 'v': float(o[5])})
        return landmarks

    # -- batch.py:253-266 -----------------------------------------------------------------------------------------
    def batch_update(self, odom_pose, dvl, landmarks: CameraMeasurement):
        """odom_pose: the Pose3 process_odom returns (:254); dvl: body-frame velocity 3-vector; landmarks: the
        CameraMeasurement message of this keyframe."""
        self.odom_accum.append(odom_pose)
        self.dvl_accum.append(np.asarray(dvl, dtype=float).reshape(3))
        self.imu_accum.append(self.imu_data)
        self.imu_data = []
        self._tf_accum.append(self.zed_world_transform)
        self.landmark_accum.append(self.get_landmarks(landmarks))

    # -- batch.py:270-305 -----------------------------------------------------------------------------------------
    def _camera_side(self):
        """Everything of batch_create except the landmark loop: priors, initial poses / velocities, IMU and DVL factors."""
        self.initial_estimate = gtsam.Values()
        self.graph = gtsam.NonlinearFactorGraph()
        self.initial_estimate.insert(B(0), self.prev_bias)                           # :274
        for i in range(len(self.odom_accum)):
            self.timestep = i
            pose = self.odom_accum[i]
            velocity = vector3(0, 0, 0)
            if i == 0:
                self.graph.add(gtsam.PriorFactorPose3(X(0), pose, self.pose_noise))  # :281
                self.graph.add(gtsam.PriorFactorVector(V(0), velocity, self.vel_noise))
                self.initial_estimate.insert(X(i), pose)
                self.initial_estimate.insert(V(i), velocity)
            else:
                self.initial_estimate.insert(X(i), pose)
                self.initial_estimate.insert(V(i), velocity)
                for imu in self.imu_accum[i]:
                    self.imu_preintegrated.integrateMeasurement(imu[:3], imu[3:], 0.005)   # :290
                self.graph.push_back(gtsam.ImuFactor(X(i - 1), V(i - 1), X(i), V(i), B(0), self.imu_preintegrated))
                self.graph.push_back(gtsam.DvlVelocityFactor(self.dvl_noise, V(i), X(i), self.dvl_accum[i]))
                self.imu_preintegrated.resetIntegration()                            # :293
                yield i

    def batch_create(self, with_landmark=True):
        """The reference's loop, object by object (batch.py:270-305)."""
        for i in self._camera_side():
            if with_landmark:
                for landmark in self.landmark_accum[i]:
                    if not self.initial_estimate.exists(L(landmark['id'])):          # :297
                        self.initial_estimate.insert(L(landmark['id']), landmark['pose'])
                    self.graph.push_back(gtsam.GenericStereoFactor3D(
                        gtsam.StereoPoint2(landmark['uL'], landmark['uR'], landmark['v']), self.landmark_noise,
                        X(i), L(landmark['id']), self.K, self.body_P_sensor))        # :300-305

    def gate_factors(self, factors, Rt: torch.Tensor, gate_px: float):
        """EXTENSION (no counterpart in batch.py, whose input has been through the nodelet's RANSAC -- here
        StereoOrbFrontend.reject_track_outliers, include/vus_ransac.h, run_sequence's ransac_px): drop every
        emitted factor whose residual AT THE INITIAL ESTIMATE -- keyframe transform Rt[f], first-sighting landmark --
        exceeds gate_px in any of (uL, uR, v) or whose landmark lies behind the camera (vus_stereo_initial_residuals).
        A brute-force Hamming mismatch is a residual of hundreds of pixels; without a robust kernel (gtsam's default,
        batch.py:118) one of them can push its landmark through a camera into the cheirality plateau.  Landmarks that
        lose every factor are dropped with them.  Returns the filtered dict (device tensors)."""
        n = factors["obs_frame"].numel()
        resid = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        K = torch.from_numpy(self.K.vector6()).to(self.device)
        from . import _lib
        ptr = _lib.ptr
        _lib.call("vus_stereo_initial_residuals", ptr(Rt), ptr(K), ptr(factors["lm_point"]), ptr(factors["obs_frame"]),
                  ptr(factors["obs_id"]), ptr(factors["obs_meas"]), n, ptr(resid), _lib.current_stream_ptr())
        keep = resid.abs().amax(1) <= float(gate_px)
        out = dict(factors)
        for k in ("obs_frame", "obs_id", "obs_meas"):
            out[k] = factors[k][keep]
        still = torch.zeros_like(factors["lm_first"], dtype=torch.bool)
        still[out["obs_id"]] = True
        out["lm_first"] = torch.where(still, factors["lm_first"], torch.full_like(factors["lm_first"], -1))
        out["initial_residuals"], out["gate_keep"] = resid, keep
        return out

    def batch_create_from_tracks(self, factors):
        """EXTENSION: the same graph from the device arrays of StereoOrbFrontend.stereo_factors() -- one
        StereoFactorBlock in batch_create's factor order, one block of first-sighting landmark values."""
        for _ in self._camera_side():
            pass
        of, oi, om = factors["obs_frame"].cpu().numpy(), factors["obs_id"].cpu().numpy(), factors["obs_meas"].cpu().numpy()
        # keys by IN-PLACE adds: `X(0) + of.astype(...)` hands numpy a large temporary, and numpy decides whether it may
        # reuse it by walking the C stack (backtrace()): with the ROCm and torch libraries loaded the first such walk of a
        # process costs ~80 ms (measured: 78 of this function's 86 ms)
        if len(of):
            kx = of.astype(np.int64)
            kx += X(0)
            kl = oi.astype(np.int64)
            kl += L(0)
            self.graph.push_back(gtsam.StereoFactorBlock(om, self.landmark_noise, kx, kl, self.K, self.body_P_sensor))
        first = factors["lm_first"].cpu().numpy()
        seen = np.nonzero(first >= 0)[0]
        if len(seen):
            ks = seen.astype(np.int64)
            ks += L(0)
            self.initial_estimate.insert_point3_block(ks, factors["lm_point"].cpu().numpy()[seen])

    def optimize(self, params: Optional["gtsam.LevenbergMarquardtParams"] = None):
        """batch.py:337."""
        self.optimizer = gtsam.LevenbergMarquardtOptimizer(self.graph, self.initial_estimate,
                                                           params or gtsam.LevenbergMarquardtParams())
        return self.optimizer.optimize()


def keyframe_transforms(odom_poses) -> np.ndarray:
    """[F,12] zed_world_transform rows (row-major R then t) from a list of Pose3 / an [F,12] array."""
    if isinstance(odom_poses, np.ndarray):
        return np.ascontiguousarray(odom_poses, dtype=np.float64).reshape(-1, 12)
    return np.stack([p.flat12() for p in odom_poses])


# Front-end settings of the end-to-end sequence: the matcher is brute force (north star), so wrong temporal matches are
# kept out by a tight Hamming bound and the mutual-match filter rather than by the nodelet's RANSAC (stereo.launch:46).
SEQUENCE_PARAMS = dict(track_max_distance=30, cross_check=True)
GATE_PX = 60.0        # 6 sigma of the stereo noise model (batch.py:118: sigma = 10 px)


def ransac_rotations(delta_body: np.ndarray, body_P_sensor: Optional["gtsam.Pose3"] = None) -> np.ndarray:
    """[P,9] R_cur_prev of vus_two_point_ransac from the BODY rotation increments delta_body [P,3,3] (R_{p+1} = R_p dR:
    what PreintegratedImuMeasurements.deltaRij() integrates from the gyro).  The camera sits at X o body_P_sensor, so
    its increment is the conjugate Rs^T dR Rs, and the map of a ray of camera p into camera p+1 its transpose."""
    Rs = np.eye(3) if body_P_sensor is None else gtsam.Pose3(body_P_sensor).rotation().matrix()
    out = [((Rs.T @ dR) @ Rs).T.reshape(-1) for dR in np.asarray(delta_body, dtype=np.float64).reshape(-1, 3, 3)]
    return np.ascontiguousarray(np.array(out, dtype=np.float64).reshape(-1, 9))


def imu_delta_rotations(imu, params: "gtsam.PreintegrationParams") -> np.ndarray:
    """[F-1,3,3] deltaRij() of every keyframe interval: the gyro samples integrated with zero bias at batch.py:290's dt."""
    pim = gtsam.PreintegratedImuMeasurements(params)
    out = []
    for smp in imu:
        pim.resetIntegration()
        for s in smp:
            s = np.asarray(s, float)
            pim.integrateMeasurement(s[:3], s[3:6], 0.005)
        out.append(pim.deltaRij().matrix())
    return np.array(out, dtype=np.float64).reshape(-1, 3, 3)


# ----------------------------------------------------------------------------------------------------------------------
# Loop closures (EXTENSION: batch.py builds an odometry-like graph only).  Candidates by pose proximity, the relative pose
# of every candidate pair by StereoOrbFrontend.match_keyframes + relative_poses (include/vus_loop.h), accepted ones as
# BetweenFactorPose3.

CANDIDATE_MODES = ("pose", "appearance", "both")
REFIT_MODES = ("left", "stereo")
NOISE_MODES = ("diagonal", "full")


@dataclass
class LoopClosureParams:
    min_gap: int = 5                    # keyframes between the two ends of a closure (neighbours are odometry's business)
    radius_m: float = 1.0               # camera centres at most this far apart in the odometry estimate
    max_angle_rad: float = 0.7          # optical axes at most this far apart
    max_per_keyframe: int = 2           # the nearest this many earlier keyframes per keyframe
    match_max_distance: int = 50        # Hamming bound of match_keyframes
    threshold_px: float = 2.0           # inlier distance of the three-point RANSAC and the refit
    n_hyp: int = 256
    seed: int = synth.SEED
    refine_iters: int = 10
    min_inliers: int = 30               # a closure with fewer final inliers is dropped
    sigma_px: float = 1.0               # floor of the residual scale s
    robust: Optional[Tuple[str, float]] = None   # e.g. ("Cauchy", 3.0): noiseModel.mEstimator name and parameter
    candidates: str = "pose"            # "pose": loop_candidates (proximity in the odometry); "appearance": appearance_candidates
                                        # on StereoOrbFrontend.keyframe_similarity (no pose enters); "both": their union
    appearance_top: int = 512           # descriptors per keyframe that take part (the strongest under global top-K)
    appearance_max_distance: int = 35   # Hamming bound of a near neighbour; tighter than match_max_distance
    appearance_min_score: int = 30      # a pair scoring less is not proposed
    # closures joining keyframes further apart stay out of the band of the reduced camera system
    # (LevenbergMarquardtParams.setLongClosureSpan); None: the band widens to them.  An init-only argument kept as a plain
    # attribute: the fields above stay the parameters of finding and measuring closures
    long_span: InitVar[Optional[int]] = None
    # The refit behind the three-point RANSAC, init-only arguments kept as plain attributes like long_span.
    # refit "left": the left-image refit of relative_poses is the measurement; "stereo": the two-view refit of
    # refine_relative_poses behind it (include/vus_pair_bundle.h), refine_iters rounds, with
    # sigma_uv_px the standard deviation of a left pixel position, sigma_disp_px that of a disparity -- None: 0.6 px with
    # integer disparities, 0.12 px with subpixel, their RMS errors within 1.5 px (profiles/subpixel.md: 0.599 and 0.120) --
    # and gate_sigma the whitened error, in sigmas, up to which a point takes part
    refit: InitVar[str] = "left"
    sigma_uv_px: InitVar[float] = 0.5
    sigma_disp_px: InitVar[Optional[float]] = None
    gate_sigma: InitVar[float] = 4.0
    # The noise model of the emitted BetweenFactorPose3, init-only and kept as a plain attribute too.  "diagonal": the
    # marginal sigmas of the measurement's covariance; "full": the whole covariance (noiseModel.Gaussian.Covariance)
    noise: InitVar[str] = "diagonal"

    def __post_init__(self, long_span=None, refit="left", sigma_uv_px=0.5, sigma_disp_px=None, gate_sigma=4.0,
                      noise="diagonal"):
        self.long_span = None if long_span is None else int(long_span)
        if self.candidates not in CANDIDATE_MODES:
            raise ValueError(f"LoopClosureParams.candidates must be one of {CANDIDATE_MODES}, not {self.candidates!r}")
        if refit not in REFIT_MODES:
            raise ValueError(f"LoopClosureParams.refit must be one of {REFIT_MODES}, not {refit!r}")
        if noise not in NOISE_MODES:
            raise ValueError(f"LoopClosureParams.noise must be one of {NOISE_MODES}, not {noise!r}")
        self.refit = refit
        self.noise = noise
        self.sigma_uv_px = float(sigma_uv_px)
        self.sigma_disp_px = None if sigma_disp_px is None else float(sigma_disp_px)
        self.gate_sigma = float(gate_sigma)

    def disparity_sigma(self, subpixel: bool) -> float:
        """sigma_disp_px, or its default for integer (False) or refined (True) disparities."""
        return float(self.sigma_disp_px) if self.sigma_disp_px is not None else (0.12 if subpixel else 0.6)


@dataclass
class SubpixelParams:
    """StereoOrbFrontend.refine_stereo (include/vus_subpixel.h): the SAD window is (2 half_win + 1)^2 pixels, shifts of
    +-search columns around the matched right keypoint are tried."""
    half_win: int = 5
    search: int = 5


def loop_candidates(poses12: np.ndarray, params: LoopClosureParams):
    """Keyframe pairs (a, b), b - a >= min_gap, whose camera centres lie within radius_m and whose optical axes (the
    camera's z axis in the world) within max_angle_rad of each other in poses12 [F,12] (camera poses, flat12).  Per b the
    max_per_keyframe nearest a, ties to the lower a; pairs ordered by b, then by distance.  Host, numpy.  Returns
    (pair_a, pair_b) int32 arrays."""
    P = np.ascontiguousarray(poses12, dtype=np.float64).reshape(-1, 12)
    centre, axis = P[:, 9:], P[:, [2, 5, 8]]
    pa, pb = [], []
    for b in range(len(P)):
        a = np.arange(0, max(b - int(params.min_gap) + 1, 0))
        if not len(a):
            continue
        dist = np.linalg.norm(centre[a] - centre[b], axis=1)
        ang = np.arccos(np.clip(axis[a] @ axis[b], -1.0, 1.0))
        ok = (dist <= params.radius_m) & (ang <= params.max_angle_rad)
        a, dist = a[ok], dist[ok]
        order = np.lexsort((a, dist))[:max(int(params.max_per_keyframe), 0)]
        pa += a[order].tolist()
        pb += [b] * len(order)
    return np.array(pa, np.int32), np.array(pb, np.int32)


def appearance_candidates(S, params: LoopClosureParams):
    """Keyframe pairs (a, b) from the similarity matrix S [F, F] of StereoOrbFrontend.keyframe_similarity (S[b, a]: how
    many of b's descriptors find a near neighbour in a): per b the a <= b - min_gap with S[b, a] >= appearance_min_score,
    of those the max_per_keyframe largest scores, ties to the lower a; pairs ordered by b, then descending score, then a.
    Host, numpy.  Returns (pair_a, pair_b) int32 arrays."""
    S = np.asarray(S.detach().cpu().numpy() if isinstance(S, torch.Tensor) else S)
    assert S.ndim == 2 and S.shape[0] == S.shape[1], "S: [F, F]"
    pa, pb = [], []
    for b in range(len(S)):
        a = np.arange(0, max(b - int(params.min_gap) + 1, 0))
        if not len(a):
            continue
        score = S[b, a].astype(np.int64)
        ok = score >= int(params.appearance_min_score)
        a, score = a[ok], score[ok]
        order = np.lexsort((a, -score))[:max(int(params.max_per_keyframe), 0)]
        pa += a[order].tolist()
        pb += [b] * len(order)
    return np.array(pa, np.int32), np.array(pb, np.int32)


def union_candidates(first, second):
    """The union of two pair lists (pair_a, pair_b) without duplicates, ordered by (b, a); int32 arrays."""
    pairs = sorted({(int(b), int(a)) for pa, pb in (first, second) for a, b in zip(pa, pb)})
    return np.array([a for _, a in pairs], np.int32), np.array([b for b, _ in pairs], np.int32)


def adjoint_map(S: "gtsam.Pose3") -> np.ndarray:
    """Ad_S in the tangent order (omega, v): S Exp(xi) S^-1 = Exp(Ad_S xi)."""
    R, t = S.rotation().matrix(), S.translation()
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    A = np.zeros((6, 6))
    A[:3, :3], A[3:, :3], A[3:, 3:] = R, tx @ R, R
    return A


def loop_closure_measurements(result, params: LoopClosureParams, body_P_sensor: Optional["gtsam.Pose3"] = None):
    """Host side of the acceptance rule: (accepted [n] bool, measured [n] Pose3 or None, cov [n,6,6], scale [n]) from a
    frontend.PairPoses.  A pair is accepted iff its status is 0 and its final inliers number at least min_inliers (and
    its normal matrix can be inverted, which three or more inliers in general position give).  cov = s^2 (JtJ)^-1,
    s = max(sigma_px, sqrt(rss / (2 n_in - 6))), in the tangent (omega, v) of measured Exp(xi).  With body_P_sensor = S
    the measurement becomes S T S^-1 (X(i) are body poses) and the covariance Ad_S cov Ad_S^T.
    From a frontend.PairBundle (refit="stereo") the count is that of the final active points, and cov = s^2 S^-1 with
    s = max(1, sqrt(chi2 / (3 n_active - 6))): S is whitened already, six residuals per point and three unknowns each."""
    T = result.T_ab.detach().cpu().numpy().reshape(-1, 12)
    info = result.info.detach().cpu().numpy().reshape(-1, 6)
    n = len(T)
    if hasattr(result, "chi2"):                    # a PairBundle
        JtJ = result.S.detach().cpu().numpy().reshape(-1, 6, 6)
        rss = result.chi2.detach().cpu().numpy().reshape(-1)
        count, status, per_point, floor = info[:, 2], info[:, 3], 3, 1.0
    else:
        JtJ = result.JtJ.detach().cpu().numpy().reshape(-1, 6, 6)
        rss = result.rss.detach().cpu().numpy().reshape(-1)
        count, status, per_point, floor = info[:, 3], info[:, 4], 2, float(params.sigma_px)
    accepted = (status == 0) & (count >= int(params.min_inliers))
    cov, scale, measured = np.zeros((n, 6, 6)), np.zeros(n), [None] * n
    S = None if body_P_sensor is None else gtsam.Pose3(body_P_sensor)
    Ad = None if S is None else adjoint_map(S)
    for c in np.nonzero(accepted)[0]:
        dof = per_point * int(count[c]) - 6
        s = max(floor, float(np.sqrt(rss[c] / dof)) if dof > 0 else 0.0)
        try:
            C = (s * s) * np.linalg.inv(JtJ[c])
        except np.linalg.LinAlgError:
            C = np.full((6, 6), np.nan)
        if not (np.isfinite(C).all() and (np.diag(C) > 0).all()):
            accepted[c] = False
            continue
        M = gtsam.Pose3.from_flat12(T[c])
        if S is not None:
            M, C = S.compose(M).compose(S.inverse()), Ad @ C @ Ad.T
        cov[c], scale[c], measured[c] = C, s, M
    return accepted, measured, cov, scale


def loop_closure_factors(result, pairs, params: LoopClosureParams, body_P_sensor: Optional["gtsam.Pose3"] = None):
    """gtsam.BetweenFactorPose3(X(a), X(b), measured, model) for every accepted pair of `result` (a frontend.PairPoses of
    pairs = (pair_a, pair_b)); see loop_closure_measurements for the rule and the covariance.  params.noise = "diagonal"
    (the default): a Diagonal model whose sigmas are the square roots of the covariance's diagonal (the marginal sigmas,
    which drop the correlation of rotation and translation: the conservative choice); "full": the whole covariance as
    noiseModel.Gaussian.Covariance(cov).  Either is wrapped in noiseModel.Robust when params.robust names an mEstimator."""
    pa, pb = (np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v).reshape(-1) for v in pairs)
    accepted, measured, cov, _ = loop_closure_measurements(result, params, body_P_sensor)
    out = []
    for c in np.nonzero(accepted)[0]:
        if params.noise == "full":
            model = gtsam.noiseModel.Gaussian.Covariance(cov[c])
        else:
            model = gtsam.noiseModel.Diagonal.Sigmas(np.sqrt(np.diag(cov[c])))
        if params.robust is not None:
            kind, k = params.robust
            model = gtsam.noiseModel.Robust.Create(getattr(gtsam.noiseModel.mEstimator, kind).Create(float(k)), model)
        out.append(gtsam.BetweenFactorPose3(X(int(pa[c])), X(int(pb[c])), measured[c], model))
    return out


def run_sequence(frames: torch.Tensor, odom_poses: np.ndarray, imu, dvl, disparity_sign: int = 1,
                 params: Optional[ImageProcessorParams] = None, bulk: bool = True, frontend: Optional[StereoOrbFrontend] = None,
                 gate_px: float = GATE_PX, body_P_sensor: Optional["gtsam.Pose3"] = None, ransac_px: float = 0.0,
                 ransac_rotation: str = "imu", rectifier=None, loop_closure: Optional[LoopClosureParams] = None,
                 subpixel: Optional[SubpixelParams] = None, enhancer=None):
    """Images to optimised trajectory: frames uint8 [F,2,H,W] on the GPU (one stereo pair per keyframe), odom_poses
    [F,12] (the odometry estimate of every keyframe = initial value of X(i) AND the camera transform get_landmarks
    uses), imu [F-1][n,>=6] samples between keyframes, dvl [F,3].  gate_px > 0 applies BatchSequence.gate_factors (bulk
    path only).  body_P_sensor: odom_poses are BODY poses, every stereo factor carries the extrinsic, and the camera
    transform of get_landmarks and of the gate is odom_pose o body_P_sensor.  ransac_px > 0 (the nodelet's
    ransac_threshold, stereo.launch:46: 3) runs StereoOrbFrontend.reject_track_outliers on the temporal matches before
    the ids are issued, with the inter-frame rotation from the gyro samples (ransac_rotation="imu": deltaRij() of every
    interval, zero bias) or from odom_poses ("odom"); stages then holds "ransac_info".  rectifier: frames are RAW camera
    images and pass through rectify.StereoRectifier.rectify first; BatchSequence keeps the reference's constant
    calibration, so the rectifier must produce that camera.  loop_closure: candidates by pose proximity in odom_poses
    (loop_candidates on the camera poses), by appearance (keyframe_similarity + appearance_candidates; stages then also holds
    "loop_similarity") or both, as LoopClosureParams.candidates says; their relative poses from the front end
    (match_keyframes + relative_poses; with LoopClosureParams.refit = "stereo" the two-view refit of refine_relative_poses
    behind it) and the accepted ones added to the graph as BetweenFactorPose3, on either path; stages then holds "loop_pairs",
    "loop_result" (None without a candidate; a PairBundle with refit = "stereo", and "loop_stage_one" then holds the
    PairPoses it started from) and "loop_accepted", and with LoopClosureParams.long_span "long_closures" (how
    many the optimiser kept out of the band).  subpixel: the stereo matches are refined on the
    (rectified) images after process() (refine_stereo) and the refined disparities replace the integer ones in the features
    of either graph builder and in the depths of the loop closures; stages then holds "stereo_disparity" (int32 [F,K], 1/256
    px) and "stereo_refine_status".  enhancer: a clahe.Clahe (anything with enhance(frames)); the frames -- rectified
    first when there is a rectifier -- pass through it before process(), and everything downstream, refine_stereo included,
    sees the enhanced images.  Returns (results Values, BatchSequence, stages dict)."""
    assert ransac_rotation in ("imu", "odom")
    if rectifier is not None:
        H, W = frames.shape[2:]
        if (np.abs(np.asarray(rectifier.camera) - default_camera(H, W)).max() > 1e-9
                or abs(rectifier.baseline - synth.BASELINE_M) > 1e-9):
            raise ValueError(f"run_sequence works with the reference's calibration: the rectifier's camera {rectifier.camera} "
                             f"and baseline {rectifier.baseline} differ from default_camera({H}, {W}) and "
                             f"{synth.BASELINE_M} -- build it with new_camera=default_camera(H, W)")
        frames = rectifier.rectify(frames)
    if enhancer is not None:
        frames = enhancer.enhance(frames)
    if params is None:
        params = ImageProcessorParams(**SEQUENCE_PARAMS)
    F, _, H, W = frames.shape
    fe = frontend or StereoOrbFrontend(H, W, max_frames=F, params=params)
    res = fe.process(frames)
    seq = BatchSequence(disparity_sign=disparity_sign, device=str(frames.device), body_P_sensor=body_P_sensor)
    Rt = keyframe_transforms(odom_poses)
    ransac_info = None
    if ransac_px > 0 and F > 1:
        if ransac_rotation == "imu":
            dR = imu_delta_rotations(imu[:F - 1], seq.PARAMS)
        else:
            Rb = Rt[:, :9].reshape(-1, 3, 3)
            dR = np.einsum("pji,pjk->pik", Rb[:-1], Rb[1:])                             # R_p^T R_{p+1}
        rot = torch.from_numpy(ransac_rotations(dR, body_P_sensor)).to(frames.device)
        ransac_info = fe.reject_track_outliers(res, rot, threshold_px=ransac_px)
    disparity = None
    if subpixel is not None:
        disparity, refine_status = fe.refine_stereo(res, frames, subpixel.half_win, subpixel.search)
    ids, feats, n_ids = fe.feature_tracks(res, disparity)
    Rt_cam = Rt if body_P_sensor is None else np.stack([gtsam.Pose3.from_flat12(r).compose(body_P_sensor).flat12() for r in Rt])
    stages = {"frontend": res, "ids": ids, "feats": feats, "n_ids": n_ids}
    if ransac_info is not None:
        stages["ransac_info"] = ransac_info
    if subpixel is not None:
        stages.update(stereo_disparity=disparity, stereo_refine_status=refine_status)
    loop_factors = []
    if loop_closure is not None:
        lc = loop_closure
        pairs = loop_candidates(Rt_cam, lc) if lc.candidates != "appearance" else None
        if lc.candidates != "pose":
            sim = fe.keyframe_similarity(res, top=lc.appearance_top, max_distance=lc.appearance_max_distance,
                                         min_gap=lc.min_gap)
            stages["loop_similarity"] = sim
            by_look = appearance_candidates(sim, lc)
            pairs = by_look if pairs is None else union_candidates(pairs, by_look)
        loop_result, accepted = None, np.zeros(0, bool)
        if len(pairs[0]):
            cam5 = np.concatenate([default_camera(H, W), [seq.baseline]])
            midx = fe.match_keyframes(res, pairs[0], pairs[1], max_distance=lc.match_max_distance)
            loop_result = fe.relative_poses(res, pairs[0], pairs[1], midx, cam5, lc.threshold_px, lc.n_hyp, lc.seed,
                                            lc.refine_iters, disparity=disparity)
            if lc.refit == "stereo":
                stages["loop_stage_one"] = loop_result
                loop_result = fe.refine_relative_poses(res, loop_result, cam5, lc.sigma_uv_px,
                                                       lc.disparity_sigma(subpixel is not None), lc.gate_sigma,
                                                       lc.refine_iters, disparity=disparity)
            accepted = loop_closure_measurements(loop_result, lc, body_P_sensor)[0]
            loop_factors = loop_closure_factors(loop_result, pairs, lc, body_P_sensor)
        stages.update(loop_pairs=pairs, loop_result=loop_result, loop_accepted=accepted)
    if bulk:
        for i in range(F):
            seq.odom_accum.append(gtsam.Pose3.from_flat12(Rt[i]))
            seq.dvl_accum.append(np.asarray(dvl[i], float))
            seq.imu_accum.append([np.asarray(s, float)[:6] for s in imu[i - 1]] if i > 0 else [])
        Rt_d = torch.from_numpy(Rt_cam).to(frames.device)
        factors = fe.stereo_factors(ids, feats, n_ids, Rt_d, seq.cam_array())
        stages["factors_ungated"] = factors
        if gate_px > 0:
            factors = seq.gate_factors(factors, Rt_d, gate_px)
        seq.batch_create_from_tracks(factors)
        stages["factors"] = factors
    else:
        msgs = fe.camera_measurements(res, disparity)
        for i in range(F):
            pose = gtsam.Pose3.from_flat12(Rt[i])
            seq.set_zed_world_transform(gtsam.Pose3.from_flat12(Rt_cam[i]).rotation(), Rt_cam[i, 9:])
            if i > 0:
                for s in imu[i - 1]:
                    seq.update_imu(s[:3], s[3:6])
            seq.batch_update(pose, dvl[i], msgs[i])
        seq.batch_create(with_landmark=True)
    for f in loop_factors:
        seq.graph.push_back(f)
    if loop_closure is None or loop_closure.long_span is None:
        return seq.optimize(), seq, stages
    lm = gtsam.LevenbergMarquardtParams()
    lm.setLongClosureSpan(loop_closure.long_span)
    results = seq.optimize(lm)
    stages["long_closures"] = seq.optimizer.report().long_closures
    return results, seq, stages
