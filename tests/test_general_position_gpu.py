"""The factor kernels on the general-position fixtures (tests/golden/general_position_*.npz: a 60-digit reference
that shares no formula with the kernels, and a bound per output block derived from that reference alone).  Reads only
the .npz files; drives vus_between_linearize / vus_between_eval_step through the C ABI, PriorFactorPose3 and the
retraction through StereoBAProblem / StereoBASolver on a graph without observations, and the stereo / mono projection
factors with PriorFactorPoint3 through StereoBAProblem (plain, loss=, body_P_sensor=, mono=) and StereoBASolver
(point_priors=), and ImuFactor / DVL / velocity priors through NavBASolver.nav_linearize / nav_eval_step."""
import numpy as np
import pytest
import torch

import general_position as gp
from visual_underwater_slam_amd import _lib

pytestmark = pytest.mark.gpu


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


POSE_CASES = [n for n in gp.case_names() if n.startswith("lie_edges")]
NAV_CASES = [n for n in gp.case_names() if n.startswith("inertial")]
PROJ_CASES = [n for n in gp.case_names() if n not in POSE_CASES + NAV_CASES]


@pytest.mark.parametrize("name", POSE_CASES)
def test_between_factors_within_the_block_bounds(gpu, name):
    from visual_underwater_slam_amd.ba import BetweenFactors
    c = gp.load_case(name)
    nP = len(c["poses"])
    B = BetweenFactors(c["btw_i"], c["btw_j"], c["btw_meas"], c["btw_sigma"], nP,
                       loss=list(zip(c["btw_kind"].tolist(), c["btw_k"].tolist())))
    band = int(np.abs(c["btw_i"] - c["btw_j"]).max())
    poses, dp, new = d(c["poses"]), d(c["dp"]), d(c["btw_new_poses"])
    lin = torch.empty((B.n, 120), dtype=torch.float64, device="cuda")
    sc = torch.zeros(4, dtype=torch.float64, device="cuda")
    work = torch.empty(int(_lib.load().vus_between_work_doubles(B.addr())), dtype=torch.float64, device="cuda")
    st, p = _lib.current_stream_ptr(), _lib.ptr
    _lib.call("vus_between_check", B.addr(), band, st)
    _lib.call("vus_between_linearize", B.addr(), p(poses), p(lin), p(sc), p(work), st)
    _lib.call("vus_between_eval_step", B.addr(), p(poses), p(dp), p(new), p(sc[1:]), p(work), st)
    out = sc.cpu().numpy()
    got = {"btw_lin": lin.cpu().numpy(), "btw_err": out[:1].reshape(1, 1), "btw_eval": out[1:3].reshape(2, 1)}
    gp.check_blocks(got, c, keys=list(got), who=f"gpu {name}")
    err = torch.zeros(1, dtype=torch.float64, device="cuda")      # vus_between_error at the new poses = the eval's second scalar
    _lib.call("vus_between_error", B.addr(), p(new), p(err), p(work), st)
    assert abs(err.item() - c["want_btw_eval"][1, 0]) <= c["tol_btw_eval"][1]


@pytest.mark.parametrize("name", POSE_CASES)
def test_pose_priors_and_retraction_within_the_block_bounds(gpu, name):
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver
    c = gp.load_case(name)
    nP = len(c["poses"])
    z = np.zeros((0,), np.int32)
    prob = StereoBAProblem(z, z, np.zeros((0, 3)), nP, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, prior_pose=c["prior_pose"],
                           prior_T=c["prior_T"], prior_sigmas=c["prior_sigma"])
    sv = StereoBASolver(prob)
    poses, points = d(c["poses"]), torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    sv.linearize(poses, points)
    sv.dp.copy_(d(c["dp"]))
    sv.eval_step(poses, points)
    sc = sv.scal.cpu().numpy()
    got = {"Hpp": sv.Hpp.cpu().numpy(), "gp": sv.gp.cpu().numpy(), "err": sc[:1].reshape(1, 1),
           "new_poses": sv.new_poses.cpu().numpy(), "eval": sc[1:3].reshape(2, 1)}
    gp.check_blocks(got, c, keys=list(got), who=f"gpu {name}")
    assert abs(sv.error(poses, points) - c["want_err"][0, 0]) <= c["tol_err"][0]


@pytest.mark.parametrize("kind", range(6))
@pytest.mark.parametrize("name", PROJ_CASES)
def test_projection_factors_within_the_block_bounds(gpu, name, kind):
    """vus_ba_linearize / _robust / _sensor / _mixed (whichever the problem selects), the landmark priors, the weights, the
    error and eval_step at the stored step, one loss kind at a time."""
    from visual_underwater_slam_amd.ba import StereoBAProblem, StereoBASolver, PointPriors
    c = gp.load_case(name)
    nP, nL = len(c["poses"]), len(c["points"])
    assert int(c["loss_kind"][kind]) == kind
    mono = bool(c["is_mono"].any())
    prob = StereoBAProblem(c["obs_pose"], c["obs_point"], c["meas"], nP, nL, c["K"][0], float(c["sigma"][0, 0]),
                           loss=(kind, float(c["loss_k"][kind, 0])) if kind else None,
                           body_P_sensor=c["sensor"][0] if len(c["sensor"]) else None, mono=c["is_mono"] if mono else None,
                           mono_K=c["mono_K"][0] if mono else None, mono_sigma=float(c["mono_sigma"][0, 0]) if mono else None)
    assert np.array_equal(prob.pk["perm"].cpu().numpy(), np.arange(len(c["obs_pose"])))      # the fixture is in L-order
    sv = StereoBASolver(prob, point_priors=PointPriors(c["pp_idx"], c["pp_mean"], c["pp_sigma"], nL))
    poses, points = d(c["poses"]), d(c["points"])
    sv.linearize(poses, points)
    sv.point_prior_linearize(points)
    sv.dp.copy_(d(c["dp"]))
    sv.dl.copy_(d(c["dl"]))
    sv.eval_step(poses, points)
    sv.point_prior_eval_step(points)
    sc = sv.scal.cpu().numpy()
    sfx = f"_k{kind}"
    got = {"W" + sfx: sv.W.cpu().numpy(), "V" + sfx: sv.V.cpu().numpy(), "gl" + sfx: sv.gl.cpu().numpy(),
           "Hpp" + sfx: sv.Hpp.cpu().numpy(), "gp" + sfx: sv.gp.cpu().numpy(), "err" + sfx: sc[:1].reshape(1, 1),
           "eval" + sfx: sc[1:3].reshape(2, 1), "weights" + sfx: sv.stereo_weights(poses, points).cpu().numpy()[:, None],
           "new_poses": sv.new_poses.cpu().numpy(), "new_points": sv.new_points.cpu().numpy()}
    if sv.Q is not None:
        pp = sv.pp_scal.cpu().numpy()
        got.update(pp_err=pp[:1].reshape(1, 1), pp_eval=pp[1:3].reshape(2, 1))
    got["error" + sfx] = np.array([[sv.error(poses, points)]])
    gp.check_blocks(got, c, keys=list(got), who=f"gpu {name}")


@pytest.mark.parametrize("name", NAV_CASES)
def test_inertial_factors_within_the_block_bounds(gpu, name):
    from visual_underwater_slam_amd.ba import StereoBAProblem, NavBASolver, NavFactors
    c = gp.load_case(name)
    nP = len(c["poses"])
    z = np.zeros((0,), np.int32)
    prob = StereoBAProblem(z, z, np.zeros((0, 3)), nP, 0, np.array([1.0, 1, 0, 0, 0, 1]), 1.0, pose_stride=2)
    nav = NavFactors(c["gravity"][0], imu=(c["imu_i"], c["imu_j"], c["imu_pim"], c["imu_W"]),
                     dvl=(c["dvl_pose"], c["dvl_meas"], c["dvl_sigma"][:, 0]), vprior=(c["vp_idx"], c["vp_v"], c["vp_sigma"]))
    sv = NavBASolver(prob, nav)
    poses, vels, bias = d(c["poses"]), d(c["vels"]), d(c["bias"][0])
    sv.nav_linearize(poses, vels, bias)
    sv.dp.copy_(d(c["dc"]))
    sv.db.copy_(d(c["db"][0]))
    sv.new_poses.copy_(d(c["new_poses"]))           # an input of vus_nav_eval_step
    sv.nav_eval_step(poses, vels, bias)
    sc = sv.nav_scal.cpu().numpy()
    got = {"Snav": sv.Snav.cpu().numpy().reshape(-1, 36), "Scb": sv.Scb.cpu().numpy(), "Sbb": sv.Sbb.cpu().numpy()[None],
           "gnav": sv.gnav.cpu().numpy(), "gb": sv.gb.cpu().numpy()[None], "nav_err": sc[:1].reshape(1, 1),
           "nav_eval": sc[1:3].reshape(2, 1), "new_vels": sv.new_vels.cpu().numpy(), "new_bias": sv.new_bias.cpu().numpy()[None]}
    gp.check_blocks(got, c, keys=list(got), who=f"gpu {name}")
    assert abs(sv.nav_error(poses, vels, bias) - c["want_nav_err"][0, 0]) <= c["tol_nav_err"][0]
