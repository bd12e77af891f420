"""The mixed stereo / monocular BA problem of the mono tests, drawn with the seeded hash generator of synth.py.

Topology (the smallest that crosses every stride of the per-observation kernels): 70 keyframes on a line, 310 landmarks;
keyframe 3 observes all 310 (> the 256 threads of lin_poses), landmark 5 is observed from all 70 keyframes (> the 64 lanes
of a lin_points wave), 310 is no multiple of the 4 points per workgroup, 70 no multiple of the 8-pose tile, every other
landmark has a track of 2-6 consecutive keyframes.  About 40 % of the observations are mono; landmark MONO_LM is mono-only
(with >= 2 sightings), keyframe MONO_KF is mono-only, landmark 5 and keyframe 3 hold both kinds.  The rows come in a
seeded shuffle, so the flags have to travel through the pack's permutation."""
import numpy as np

from visual_underwater_slam_amd import synth
import mono_ref

N_KF, N_LM = 70, 310
MONO_LM, MONO_KF, STEREO_LM = 11, 40, 7
SEED = synth.SEED ^ 0x4D4F4E4F


def mono_calibration(K):
    """a Cal3_S2 of its own, skew included: (fx, fy, s, cx, cy)"""
    return np.array([1.01 * K[0], 0.99 * K[1], 1.5, K[3] + 3.0, K[4] - 2.0])


def stereo_project(T, p, K):
    q = T[:9].reshape(3, 3).T @ (p - T[9:])
    return np.array([K[3] + K[0] * q[0] / q[2], K[3] + K[0] * (q[0] - K[5]) / q[2], K[4] + K[1] * q[1] / q[2]]), q[2]


def mixed_sequence(mono_frac=0.4, n_kf=N_KF, n_lm=N_LM, mono_K=None, mono_sigma=7.0, outliers=0.0, seed=SEED):
    """dict like synth.ba_sequence's plus `mono` (bool per row), `mono_K`, `mono_sigma`; a mono row's meas is
    (u, NaN, v).  mono_frac = 0: all stereo; 1: all mono.  outliers: that fraction of rows shifted 50-300 px along u (uL and uR together)."""
    fx, fy, cx, cy = synth.INTRINSIC
    K = np.array([fx, fy, 0.0, cx, cy, synth.BASELINE_M])
    mono_K = mono_calibration(K) if mono_K is None else np.asarray(mono_K, float)
    U = synth._hash_uniform
    poses = np.zeros((n_kf, 12))
    for i in range(n_kf):
        poses[i, :9] = synth._rodrigues(np.array([0.05 * np.sin(0.7 * i), 0.04 * np.cos(0.4 * i), 0.1 * np.sin(0.3 * i)])).reshape(-1)
        poses[i, 9:] = (0.1 * i, 0.05 * np.sin(0.5 * i), 0.0)
    j = np.arange(n_lm, dtype=np.int64)
    length = 2 + (5 * U(j, seed ^ 0x0101)).astype(np.int64)                # 2..6
    start = ((n_kf - length + 1) * U(j, seed ^ 0x0202)).astype(np.int64)
    pts = np.stack([0.1 * (start + 0.5 * length) - 1.0 + 2.0 * U(j, seed ^ 0x0303), -1.0 + 2.0 * U(j, seed ^ 0x0404),
                    3.0 + 3.0 * U(j, seed ^ 0x0505)], 1)
    if n_lm > 5:
        pts[5] = (0.05 * n_kf, 0.1, 5.0)
    pairs = set()
    for l in range(n_lm):
        for i in range(int(start[l]), int(start[l] + length[l])):
            pairs.add((l, i))
        if n_kf > 3:
            pairs.add((l, 3))
    if n_lm > 5:
        pairs.update((5, i) for i in range(n_kf))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    n = len(pairs)
    a = np.arange(n, dtype=np.int64)
    order = np.argsort(U(a, seed ^ 0x0606), kind="stable")                  # rows in a seeded shuffle
    obs_l, obs_p = pairs[order, 0], pairs[order, 1]
    mono = U(a, seed ^ 0x0707) < mono_frac
    if 0.0 < mono_frac < 1.0:
        mono[obs_l == MONO_LM] = True
        mono[obs_p == MONO_KF] = True
        mono[obs_l == STEREO_LM] = False
    noise = synth._hash_normal(3 * n, seed ^ 0x0808).reshape(n, 3)
    off = np.zeros(n)
    if outliers:
        # only on landmarks with at least five sightings: one gross outlier among two or three sightings leaves a
        # redescending loss free to send the landmark to infinity, which is a property of such a graph, not of the solver
        rank = np.argsort(U(a, seed ^ 0x0909), kind="stable")
        rank = rank[np.bincount(obs_l, minlength=n_lm)[obs_l[rank]] >= 5]
        out = np.zeros(n, bool)
        out[rank[:int(round(outliers * n))]] = True
        off = np.where(out, np.where(U(a, seed ^ 0x0A0A) < 0.5, -1.0, 1.0) * (50.0 + 250.0 * U(a, seed ^ 0x0B0B)), 0.0)
    meas = np.empty((n, 3))
    for r in range(n):
        T, p = poses[obs_p[r]], pts[obs_l[r]]
        if mono[r]:
            uv, z = mono_ref.mono_project(T, p, mono_K)
            meas[r] = (uv[0] + noise[r, 0] + off[r], np.nan, uv[1] + noise[r, 2])
        else:
            m, z = stereo_project(T, p, K)
            meas[r] = m + noise[r] + (off[r], off[r], 0.0)
        assert z > 1.0
    poses_init = poses.copy()
    nt = 0.05 * synth._hash_normal(3 * n_kf, seed ^ 0x0C0C).reshape(n_kf, 3)
    nr = 0.01 * synth._hash_normal(3 * n_kf, seed ^ 0x0D0D).reshape(n_kf, 3)
    for i in range(1, n_kf):
        poses_init[i, :9] = (poses[i, :9].reshape(3, 3) @ synth._rodrigues(nr[i])).reshape(-1)
        poses_init[i, 9:] = poses[i, 9:] + nt[i]
    pts_init = pts + 0.05 * synth._hash_normal(3 * n_lm, seed ^ 0x0E0E).reshape(n_lm, 3)
    return {"poses_gt": poses, "poses_init": poses_init, "points_gt": pts, "points_init": pts_init,
            "obs_pose": obs_p.astype(np.int32), "obs_point": obs_l.astype(np.int32), "meas": meas, "K": K,
            "sigma": synth.STEREO_SIGMA, "prior_sigmas": np.array(synth.PRIOR_SIGMAS), "mono": mono, "mono_K": mono_K,
            "mono_sigma": float(mono_sigma)}


def check_topology(seq):
    """the properties the tests rely on"""
    p, l, m = seq["obs_pose"], seq["obs_point"], seq["mono"]
    assert len(seq["poses_gt"]) == 70 and len(seq["points_gt"]) == 310
    assert (p == 3).sum() == 310 and (l == 5).sum() == 70
    per_lm = np.bincount(l, minlength=310)
    assert per_lm.min() >= 2
    assert 0.3 < m.mean() < 0.5
    for sel in (l == 5, p == 3):
        assert m[sel].any() and (~m[sel]).any()
    assert m[l == MONO_LM].all() and (l == MONO_LM).sum() >= 2
    assert m[p == MONO_KF].all() and (p == MONO_KF).sum() >= 1
    assert not m[l == STEREO_LM].any()
    assert np.isnan(seq["meas"][m, 1]).all() and np.isfinite(seq["meas"][~m]).all()
    assert np.isfinite(seq["meas"][:, [0, 2]]).all()
