"""The f64 CPU twins (the oracle's factors under the numpy references between_ref, point_prior_ref, mono_ref, sensor_ref,
robust_ref) on the general-position fixtures of tests/golden/make_general_position.py: every block of every output within the bound the 60-digit reference derived for it
(32 x the change that rounding the inputs causes + 32 eps max|block|), never a relative error over a whole array.  This
is what shows that an f64 implementation can meet the bounds the GPU file applies to the kernels."""
import importlib.util
import os

import numpy as np
import pytest

import general_position as gp


@pytest.mark.parametrize("name", gp.case_names())
def test_cpu_twins_within_the_block_bounds(oracle, name):
    c = gp.load_case(name)
    for sig, w in (("btw_sigma", "btw_w"), ("prior_sigma", "prior_w"), ("sigma", "inv_sigma"), ("mono_sigma", "mono_w"), ("pp_sigma", "pp_w"),
                   ("dvl_sigma", "dvl_w"), ("vp_sigma", "vp_w")):
        assert sig not in c or np.array_equal(1.0 / c[sig], c[w])        # the reference read w, the classes are given sigma
    assert os.path.getsize(os.path.join(gp.GOLDEN, f"general_position_{name}.npz")) < 349157
    r = gp.check_blocks(gp.oracle_outputs(oracle, c), c, who=f"oracle {name}")
    for k, v in r.items():          # the figure recorded when the fixture was made (libm may move it by an ulp or two)
        assert v <= max(2.0 * float(c["oracle_ratio_" + k]), 0.25), (k, v, float(c["oracle_ratio_" + k]))


@pytest.mark.parametrize("name", ["lie_edges_a", "lie_edges_b"])
def test_gtsam_shim_pose3_within_the_block_bounds(name):
    """Pose3.localCoordinates / retract of the gtsam shim (host numpy, the kernels' conventions) on the pose cases: the
    prior gradient w^2 Log(T^-1 prior) and the retracted poses."""
    from visual_underwater_slam_amd.gtsam import Pose3
    c = gp.load_case(name)
    P = [Pose3.from_flat12(T) for T in c["poses"]]
    got = {"gp": np.stack([-c["prior_w"][q] ** 2 * P[i].localCoordinates(Pose3.from_flat12(c["prior_T"][q]))
                           for q, i in enumerate(c["prior_pose"])]),
           "new_poses": np.stack([P[i].retract(c["dp"][i]).flat12() for i in range(len(P))])}
    assert np.array_equal(c["prior_pose"], np.arange(len(P)))
    gp.check_blocks(got, c, keys=list(got), who=f"gtsam shim {name}")


def test_cases_cover_every_branch_of_log_and_exp():
    """The residual rotations of the between factors as stored: 0, below Logmap's th < 1e-10, either side of kEps, of the
    Jacobian switch, of the tr - 3 < -1e-7 switch, mid range and six angles in the last 1e-2 before pi."""
    want = [0, 5e-11, 1e-9, 1.4e-8, 1.6e-8, 9e-6, 1.1e-5, 3.0e-4, 3.3e-4, 1, 2.5] + [np.pi - x for x in (1e-2, 1e-3, 1e-4, 2e-5, 9e-6, 5e-6)]
    for name in ("lie_edges_a", "lie_edges_b"):
        c = gp.load_case(name)
        assert len(c["poses"]) <= 8 and len(c["btw_i"]) == len(want)
        assert sorted(set(c["btw_kind"].tolist())) == [0, 1, 2, 3, 4, 5]
        steps = np.linalg.norm(c["dp"][:, :3], axis=1)
        assert np.abs(c["dp"][:, 3:]).max() > 100 and np.abs(c["btw_meas"][:, 9:]).max() > 100      # translations up to 1e3
        assert steps.max() > np.pi - 1e-3 if name == "lie_edges_a" else steps.max() > np.pi - 6e-6


def test_projection_cases_hold_what_they_are_for():
    """Cheirality rows (one exactly on the plane z = 0), a single sighting, a mono-only landmark, residuals on both sides
    of k, the far offset, the extrinsic."""
    for name in ("attitudes", "far_origin", "calibration", "attitudes_sensor", "far_origin_sensor", "calibration_sensor"):
        c = gp.load_case(name)
        nO = len(c["obs_pose"])
        assert len(c["poses"]) <= 8 and len(c["points"]) <= 40 and nO <= 160
        assert np.array_equal(np.lexsort((c["obs_pose"], c["obs_point"])), np.arange(nO))                # L-order
        per_lm = np.bincount(c["obs_point"])
        assert per_lm.min() == 1 and per_lm.max() >= 4
        w_huber, w_tukey = c["want_weights_k1"][:, 0], c["want_weights_k3"][:, 0]
        assert 0.25 * nO < (w_huber == 1.0).sum() < 0.75 * nO and 0.25 * nO < (w_tukey == 0.0).sum() < 0.75 * nO
        cheiral = np.abs(c["want_W_k0"]).max(axis=1) == 0.0
        assert cheiral.sum() >= 3 and cheiral[c["obs_point"] == 2].all() and 0 < cheiral[c["obs_point"] == 1].sum() < per_lm[1]
        assert (len(c["sensor"]) == 1) == name.endswith("_sensor")
        if name == "attitudes":
            a = np.nonzero((c["obs_point"] == 0) & (c["obs_pose"] == 0))[0][0]
            assert cheiral[a] and c["points"][0, 2] == 0.0 and np.array_equal(c["poses"][0], np.eye(4)[:3].T.reshape(-1)[:12])
        if name.startswith("far_origin"):
            assert np.abs(c["points"][:, 1]).min() > 5e6
        if name.startswith("calibration"):
            mono = c["is_mono"] != 0
            assert 0.3 * nO < mono.sum() < 0.5 * nO and mono[c["obs_point"] == 4].all() and c["mono_K"][0, 2] != 0.0
            assert len(c["pp_idx"]) >= 2 and c["K"][0, 0] != c["K"][0, 1]


def test_inertial_cases_hold_what_they_are_for():
    """Rotation residuals of 0.5 rad and pi - 1e-3, gyro-bias deltas 0, 1e-6 and 0.05 rad/s in `inertial`; residuals and
    phi = dR_dbg dbg on either side of the SO(3) Jacobians' th2 < 1e-10 switch and of kEps in `inertial_edges`."""
    def sizes(c):
        import nav_ref    # noqa: F401  (the layouts are nav_ref's)
        dbg = c["bias"][0, 3:] - c["imu_pim"][:, 64:67]
        phi = np.einsum("fij,fj->fi", c["imu_pim"][:, 16:25].reshape(-1, 3, 3), dbg)
        return np.linalg.norm(dbg, axis=1), np.linalg.norm(phi, axis=1)
    c = gp.load_case("inertial")
    dbg, _ = sizes(c)
    assert len(c["poses"]) == 4 and len(c["dvl_pose"]) == 4 and dbg[0] == 0.0
    assert abs(dbg[1] - 1e-6) < 1e-12 and abs(dbg[2] - 0.05) < 1e-12
    assert abs(np.linalg.norm(c["gravity"][0]) - 9.8) < 0.1 and np.abs(c["gravity"][0]).min() > 0.5
    c = gp.load_case("inertial_edges")
    _, phi = sizes(c)
    assert len(c["poses"]) == 8 and phi.min() == 0.0
    for lo, hi in ((8e-6, 1e-5), (1e-5, 1.2e-5), (1e-8, 1.49e-8), (1.49e-8, 2e-8)):
        assert ((phi > lo) & (phi < hi)).any(), (lo, hi, phi)


def test_generator_reproduces_a_committed_case_bit_for_bit():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_general_position", os.path.join(gp.GOLDEN, "make_general_position.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c, new = gp.load_case("lie_edges_a"), gen.build_case("lie_edges_a")
    for k, v in new.items():
        a, b = np.asarray(v), c[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
