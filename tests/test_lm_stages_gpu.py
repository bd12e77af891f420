"""The LM stages of ba.py are written once, in StereoBASolver, over the solver's list of factor terms (between factors,
landmark priors, inertial factors, in that order) and one trial record.  On the smallest graph of synth.nav_sequence
(4 keyframes, 11 landmarks) every solver class with every combination of optional families runs one linearisation, one
solve and one step evaluation under a recorder of the library calls: which entry points each stage calls, the order
constraints between them, the layout of the trial record, and the error sums in the record's association."""
import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth
import between_ref as br
import nav_bias_ref as nbr

pytestmark = pytest.mark.gpu

LAM = 1e-3
# (solver, between, landmark priors) -> the entry points of the linearise, solve and evaluate stages, from the call lists
# of the stage methods before they were merged; the band solve's name is completed by the case's use_split
CASES = {
    ("stereo", False, False): (["vus_ba_linearize"],
                               ["vus_ba_schur", "vus_ba_band_solve", "vus_ba_backsub"],
                               ["vus_ba_eval_step"]),
    ("stereo", True, False): (["vus_ba_linearize", "vus_between_linearize"],
                              ["vus_ba_schur", "vus_between_assemble", "vus_ba_band_solve", "vus_ba_backsub"],
                              ["vus_ba_eval_step", "vus_between_eval_step"]),
    ("stereo", False, True): (["vus_ba_linearize", "vus_point_prior_linearize"],
                              ["vus_ba_schur", "vus_ba_band_solve", "vus_ba_backsub"],
                              ["vus_ba_eval_step", "vus_point_prior_eval_step"]),
    ("stereo", True, True): (["vus_ba_linearize", "vus_between_linearize", "vus_point_prior_linearize"],
                             ["vus_ba_schur", "vus_between_assemble", "vus_ba_band_solve", "vus_ba_backsub"],
                             ["vus_ba_eval_step", "vus_between_eval_step", "vus_point_prior_eval_step"]),
    ("nav", False, False): (["vus_ba_linearize", "vus_nav_linearize"],
                            ["vus_ba_schur", "vus_nav_assemble", "vus_ba_band_solve_multi", "vus_nav_border_solve",
                             "vus_ba_backsub"],
                            ["vus_ba_eval_step", "vus_nav_eval_step"]),
    ("nav", True, True): (["vus_ba_linearize", "vus_between_linearize", "vus_point_prior_linearize", "vus_nav_linearize"],
                          ["vus_ba_schur", "vus_between_assemble", "vus_nav_assemble", "vus_ba_band_solve_multi",
                           "vus_nav_border_solve", "vus_ba_backsub"],
                          ["vus_ba_eval_step", "vus_between_eval_step", "vus_point_prior_eval_step", "vus_nav_eval_step"]),
    ("navb", True, True): (["vus_ba_linearize", "vus_between_linearize", "vus_point_prior_linearize", "vus_navb_linearize"],
                           ["vus_ba_schur", "vus_between_assemble", "vus_navb_assemble", "vus_ba_band_solve", "vus_ba_backsub"],
                           ["vus_ba_eval_step", "vus_between_eval_step", "vus_point_prior_eval_step", "vus_navb_eval_step"]),
}
STRIDE = {"stereo": 1, "nav": 2, "navb": 3}


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_seq = {}


def _sequence():
    """the sequence and its IMU preintegration, computed once and shared (read only)"""
    if not _seq:
        s = synth.nav_sequence(4, 50, 20)
        _seq.update(s=s, pim=nbr.preintegrate(s))
    return _seq["s"], _seq["pim"]


def _build(kind, with_between, with_priors):
    """(solver, LM state) of one case"""
    from visual_underwater_slam_amd import ba
    from visual_underwater_slam_amd.gtsam import Pose3
    s, (pims, Ws) = _sequence()
    n, nL = len(s["poses_gt"]), len(s["points_gt"])
    assert (n, nL) == (4, 11)
    stride = STRIDE[kind]
    between = priors = None
    if with_between:            # odometry and one closure, both key orders
        pairs = [(0, 1), (2, 1), (2, 3), (3, 0)]
        T = [Pose3.from_flat12(x) for x in s["poses_gt"]]
        G = br.BetweenSet([a for a, _ in pairs], [b for _, b in pairs], np.array([T[a].between(T[b]).flat12() for a, b in pairs]),
                          np.tile((0.01, 0.01, 0.01, 0.05, 0.05, 0.05), (len(pairs), 1)))
        between = G.device(n, stride)
    if with_priors:             # first and last landmark, two priors on one landmark, not sorted
        idx = np.array([nL - 1, 4, 0, 4])
        priors = ba.PointPriors(idx, s["points_gt"][idx] + np.array([0.1, -0.2, 0.3]), np.tile((0.3, 0.05, 0.7), (4, 1)), nL)
    prob = ba.StereoBAProblem(s["obs_pose"], s["obs_point"], s["meas"], n, nL, s["K"], s["sigma"], prior_pose=[0],
                              prior_T=s["poses_gt"][:1], prior_sigmas=s["prior_sigmas"][None], pose_stride=stride,
                              between_span=3 if with_between else 0)
    poses, points, vels = d(s["poses_init"]), d(s["points_init"]), d(np.zeros((n, 3)))
    if kind == "stereo":
        return ba.StereoBASolver(prob, between, priors), (poses, points)
    dvl = (np.arange(1, n), s["dvl"][1:], np.full(n - 1, 0.1))
    vprior = (np.array([0]), np.zeros((1, 3)), np.full((1, 3), 0.1))
    if kind == "nav":
        nav = ba.NavFactors(s["gravity"], imu=(np.arange(n - 1), np.arange(1, n), pims, Ws), dvl=dvl, vprior=vprior)
        return ba.NavBASolver(prob, nav, between, priors), (poses, vels, d(np.zeros(6)), points)
    G = nbr.BiasGraph(s["gravity"], imu=(np.arange(n - 1), pims, Ws), dvl=dvl, vprior=vprior,
                      bbetween=(np.arange(n - 1), np.zeros((n - 1, 6)), np.full((n - 1, 6), 1e-3)),
                      bprior=(np.array([0]), np.zeros((1, 6)), np.full((1, 6), 0.1)))
    return ba.NavBiasBASolver(prob, G.device(), between, priors), (poses, vels, d(np.zeros((n, 6))), points)


@pytest.mark.parametrize("kind,with_between,with_priors", list(CASES), ids=lambda v: str(v))
def test_stages_call_the_terms_in_order_and_share_one_record(gpu, monkeypatch, kind, with_between, with_priors):
    from visual_underwater_slam_amd import _lib
    sv, state = _build(kind, with_between, with_priors)
    calls = []
    through = _lib.call

    def recorder(name, *args):
        calls.append(name)
        return through(name, *args)
    monkeypatch.setattr(_lib, "call", recorder)

    def recorded(stage, *args):
        del calls[:]
        out = stage(*args)
        return list(calls), out

    lin, _ = recorded(sv._lm_linearize, state)
    solve, _ = recorded(sv._lm_solve, LAM)
    ev, (status, errs) = recorded(sv._lm_eval, state)
    lin_all, _ = recorded(sv._linearize_all, state)           # the marginals' linearisation: the same, then the check
    zero, _ = recorded(sv._assemble_zero)
    monkeypatch.undo()
    print(f"{kind} between={with_between} priors={with_priors}:\n  {lin}\n  {solve}\n  {ev}\n  {lin_all}\n  {zero}")

    # 1. exactly the entry points of the case
    want_lin, want_solve, want_ev = CASES[kind, with_between, with_priors]
    if sv.use_split:
        want_solve = [x + "_split" if x.startswith("vus_ba_band_solve") else x for x in want_solve]
    assert sorted(lin) == sorted(want_lin) and sorted(solve) == sorted(want_solve) and sorted(ev) == sorted(want_ev)
    assert sorted(lin_all) == sorted(want_lin + ["vus_ba_point_check"])
    n_assemble = 1 + with_between + (kind != "stereo")
    assert sorted(zero) == sorted(want_solve[:n_assemble])

    # 2. the order constraints
    if with_priors:         # the stereo linearisation first: the priors add into its V and gl; both before the check
        assert lin.index("vus_ba_linearize") < lin.index("vus_point_prior_linearize")
        assert lin_all.index("vus_ba_linearize") < lin_all.index("vus_point_prior_linearize") < lin_all.index("vus_ba_point_check")
    assert lin_all[-1] == "vus_ba_point_check"
    for seq in (solve, zero):
        assert seq[0] == "vus_ba_schur"                      # (and every linearisation ran in the stage before it)
        if with_between:
            assert seq[1] == "vus_between_assemble"          # after schur, before an inertial assemble copies gs
        if kind != "stereo":
            assert seq[n_assemble - 1] == f"vus_{kind}_assemble"
    assert solve[-1] == "vus_ba_backsub"
    assert ev[0] == "vus_ba_eval_step"                       # the others read new_poses / new_points

    # 3. one record: 5 doubles and a slot of 4 per term, in the order between, landmark priors, inertial
    views = [name for name, present in (("btw_scal", with_between), ("pp_scal", with_priors), ("nav_scal", kind != "stereo"))
             if present]
    assert len(sv._terms) == len(views) and sv._trial.numel() == 5 + 4 * len(views)
    assert sv.scal.data_ptr() == sv._trial.data_ptr() and sv.status.data_ptr() == sv._trial[4:].data_ptr()
    for name in ("btw_scal", "pp_scal", "nav_scal"):
        assert hasattr(sv, name) == (name in views)

    # 4. the errors of the trial: stereo + between + priors + inertial, read from the views, exactly
    assert status == 0
    parts = [sv.scal.cpu()] + [getattr(sv, name).cpu() for name in views]
    for k in range(3):
        want = float(parts[0][k])
        for part in parts[1:]:
            want = want + float(part[k])
        print(f"  errs[{k}] = {errs[k]!r}, from the views {want!r}")
        assert np.isfinite(want) and want > 0.0 and errs[k] == want
    if kind != "stereo":
        assert sv.nav_scal.numel() == 4

    # 5. the views alias the record: written through the view, read back from the record
    for i, name in enumerate(views):
        view = getattr(sv, name)
        assert sv._terms[i].scal.data_ptr() == view.data_ptr() == sv._trial[5 + 4 * i:].data_ptr()
        view[2] = 1000.0 + i
        assert float(sv._trial[5 + 4 * i + 2]) == 1000.0 + i
        sv._trial[5 + 4 * i + 1] = -7.0 - i
        assert float(view[1]) == -7.0 - i
