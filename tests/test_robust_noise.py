"""Robust noise models of the stereo factors, CPU side: the gtsam.noiseModel.mEstimator closed forms, the
noiseModel.Robust plumbing of the gtsam shim and graph packing, the C ABI's host-side validation, and the numpy
reference (tests/robust_ref.py) against the oracle's Gaussian LM."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from visual_underwater_slam_amd import synth, ba_pack, gtsam
from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L, V
from visual_underwater_slam_amd.gtsam.optimizer import _pack_graph
import robust_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ME = gtsam.noiseModel.mEstimator
K_PAR = 1.345


def _table(name, k, d):
    """The issue's table, case by case (independent of both the shim and robust_ref)."""
    if name == "Huber":
        return (1.0, d * d / 2) if d <= k else (k / d, k * d - k * k / 2)
    if name == "Cauchy":
        return k * k / (k * k + d * d), (k * k / 2) * math.log(1 + d * d / (k * k))
    if name == "Tukey":
        return ((1 - d * d / (k * k)) ** 2, (k * k / 6) * (1 - (1 - d * d / (k * k)) ** 3)) if d <= k else (0.0, k * k / 6)
    if name == "GemanMcClure":
        return k ** 4 / (k * k + d * d) ** 2, (k * k / 2) * d * d / (k * k + d * d)
    if name == "Welsch":
        return math.exp(-d * d / (k * k)), (k * k / 2) * (1 - math.exp(-d * d / (k * k)))
    raise ValueError(name)


NAMES = ("Huber", "Cauchy", "Tukey", "GemanMcClure", "Welsch")


@pytest.mark.parametrize("name", NAMES)
def test_mestimator_closed_forms(name):
    est = getattr(ME, name).Create(K_PAR)
    kind = robust_ref.KINDS[{"GemanMcClure": "geman_mcclure"}.get(name, name.lower())]
    assert est.kind == kind and est.k == K_PAR
    for d in (0.0, K_PAR / 2, K_PAR, 2 * K_PAR, 10 * K_PAR):
        w, rho = _table(name, K_PAR, d)
        assert est.weight(d) == pytest.approx(w, rel=1e-14, abs=1e-300)
        assert est.sqrtWeight(d) == pytest.approx(math.sqrt(w), rel=1e-14, abs=1e-300)
        assert est.loss(d) == pytest.approx(rho, rel=1e-13, abs=1e-300)
        rw, rr = robust_ref.weight_loss(kind, K_PAR, np.array([d]))
        assert rw[0] == pytest.approx(w, rel=1e-14, abs=1e-300) and rr[0] == pytest.approx(rho, rel=1e-13, abs=1e-300)
    assert est.weight(0.0) == 1.0 and est.loss(0.0) == 0.0


@pytest.mark.parametrize("name", ("Huber", "Tukey"))
def test_piecewise_losses_are_continuous_at_k(name):
    est = getattr(ME, name).Create(K_PAR)
    eps = 1e-9
    assert abs(est.loss(K_PAR - eps) - est.loss(K_PAR + eps)) < 1e-8
    assert abs(est.weight(K_PAR - eps) - est.weight(K_PAR + eps)) < 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_irls_identity(name):
    """rho'(d) = d w(d): the weight IS the IRLS weight of the loss."""
    est = getattr(ME, name).Create(K_PAR)
    for d in (0.3 * K_PAR, 0.8 * K_PAR, 1.7 * K_PAR, 4.0 * K_PAR):
        if name == "Tukey" and d > K_PAR:
            assert est.weight(d) == 0.0
        h = 1e-6 * d
        deriv = (est.loss(d + h) - est.loss(d - h)) / (2 * h)
        assert deriv == pytest.approx(d * est.weight(d), rel=1e-7, abs=1e-9)


def test_mestimator_rejects_bad_parameters():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError):
            ME.Huber.Create(bad)
    with pytest.raises(NotImplementedError):
        ME.Cauchy.Create(1.0, "Scalar")


def _stereo_graph(model, n_kf=6, n_lm=60, obs=20, block=False, prior_model=None):
    seq = synth.ba_sequence(n_kf, n_lm, obs)
    nL = len(seq["points_gt"])
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    graph.add(gtsam.PriorFactorPose3(X(0), gtsam.Pose3.from_flat12(seq["poses_init"][0]),
                                     prior_model or gtsam.noiseModel.Diagonal.Sigmas(seq["prior_sigmas"])))
    K = gtsam.Cal3_S2Stereo(*seq["K"])
    for i in range(n_kf):
        values.insert(X(i), gtsam.Pose3.from_flat12(seq["poses_init"][i]))
    for j in range(nL):
        values.insert(L(j), seq["points_init"][j])
    if block:
        graph.push_back(gtsam.StereoFactorBlock(seq["meas"], model, [X(int(i)) for i in seq["obs_pose"]],
                                                [L(int(j)) for j in seq["obs_point"]], K))
    else:
        for a in range(len(seq["obs_pose"])):
            graph.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*seq["meas"][a]), model,
                                                        X(int(seq["obs_pose"][a])), L(int(seq["obs_point"][a])), K))
    return seq, graph, values


def test_robust_create_wraps_an_isotropic_model():
    base = gtsam.noiseModel.Isotropic.Sigma(3, 10.0)
    est = ME.Huber.Create(K_PAR)
    n = gtsam.noiseModel.Robust.Create(est, base)
    assert n.dim() == 3 and n.noise() is base and n.robust() is est
    assert n.is_isotropic() and np.array_equal(n.sigmas(), [10.0, 10.0, 10.0])
    with pytest.raises(RuntimeError):
        gtsam.noiseModel.Robust.Create(base, base)


@pytest.mark.parametrize("block", (False, True))
@pytest.mark.parametrize("name", ("Huber", "Welsch"))
def test_pack_graph_carries_the_loss(block, name):
    est = getattr(ME, name).Create(2.5)
    model = gtsam.noiseModel.Robust.Create(est, gtsam.noiseModel.Isotropic.Sigma(3, 10.0))
    seq, graph, values = _stereo_graph(model, block=block)
    pg = _pack_graph(graph, values, device=None)
    assert pg["sigma"] == 10.0 and pg["loss"] == (est.kind, 2.5)
    assert len(pg["meas"]) == len(seq["meas"])
    # the Gaussian graph packs without a loss, as before
    _, g2, v2 = _stereo_graph(gtsam.noiseModel.Isotropic.Sigma(3, 10.0), block=block)
    assert _pack_graph(g2, v2, device=None)["loss"] is None


def test_mixed_stereo_models_are_refused():
    iso = gtsam.noiseModel.Isotropic.Sigma(3, 10.0)
    seq, graph, values = _stereo_graph(gtsam.noiseModel.Robust.Create(ME.Cauchy.Create(2.0), iso))
    K = gtsam.Cal3_S2Stereo(*seq["K"])
    for other in (iso, gtsam.noiseModel.Robust.Create(ME.Cauchy.Create(3.0), iso),
                  gtsam.noiseModel.Robust.Create(ME.Huber.Create(2.0), iso)):
        g = gtsam.NonlinearFactorGraph()
        for f in graph._factors:
            g.push_back(f)
        g.push_back(gtsam.GenericStereoFactor3D(gtsam.StereoPoint2(*seq["meas"][0]), other, X(0), L(0), K))
        with pytest.raises(NotImplementedError, match="share one noise model"):
            _pack_graph(g, values, device=None)
    # a block with another model than the single factors
    g = gtsam.NonlinearFactorGraph()
    for f in graph._factors:
        g.push_back(f)
    g.push_back(gtsam.StereoFactorBlock(seq["meas"][:3], iso, [X(0)] * 3, [L(0)] * 3, K))
    with pytest.raises(NotImplementedError, match="share one noise model"):
        _pack_graph(g, values, device=None)


def test_robust_models_on_other_factors_are_refused():
    rob6 = gtsam.noiseModel.Robust.Create(ME.Huber.Create(1.0), gtsam.noiseModel.Isotropic.Sigma(6, 0.1))
    rob3 = gtsam.noiseModel.Robust.Create(ME.Huber.Create(1.0), gtsam.noiseModel.Isotropic.Sigma(3, 0.1))
    with pytest.raises(NotImplementedError, match="stereo factors only"):
        gtsam.PriorFactorPose3(X(0), gtsam.Pose3(), rob6)
    with pytest.raises(NotImplementedError, match="stereo factors only"):
        gtsam.PriorFactorVector(V(0), np.zeros(3), rob3)
    with pytest.raises(NotImplementedError, match="stereo factors only"):
        gtsam.DvlVelocityFactor(rob3, V(0), X(0), np.zeros(3))


def test_robust_entry_points_are_exported_bound_and_validate_the_loss():
    """include/vus_robust.h (included by vus.h): every entry point exported and bound; the loss is checked on the host
    before anything is launched."""
    import re
    import visual_underwater_slam_amd._lib as Lb
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vus_robust.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vus_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["vus_ba_error_robust", "vus_ba_eval_step_robust", "vus_ba_linearize_robust", "vus_ba_stereo_weights"]
    assert '#include "vus_robust.h"' in open(os.path.join(ROOT, "include", "vus.h")).read()
    lib = Lb.load()
    for n in names:
        assert n in Lb.SIGNATURES and hasattr(lib, n)

    class Loss(ctypes.Structure):
        _fields_ = [("kind", ctypes.c_int), ("k", ctypes.c_double)]
    p8 = ctypes.c_void_p(8)
    for loss, msg in ((None, b"loss is null"), (Loss(6, 1.0), b"unknown loss kind"), (Loss(-1, 1.0), b"unknown loss kind"),
                      (Loss(1, 0.0), b"must be finite"), (Loss(2, -1.0), b"must be finite"),
                      (Loss(3, float("inf")), b"must be finite"), (Loss(4, float("nan")), b"must be finite")):
        ref = ctypes.byref(loss) if loss is not None else None
        assert lib.vus_ba_error_robust(p8, p8, p8, p8, p8, None, ref) == -1 and msg in lib.vus_last_error()
        assert lib.vus_ba_stereo_weights(p8, ref, p8, p8, p8, None) == -1 and msg in lib.vus_last_error()
        assert lib.vus_ba_linearize_robust(p8, p8, p8, p8, p8, p8, p8, p8, p8, p8, None, ref) == -1
        assert lib.vus_ba_eval_step_robust(p8, p8, p8, p8, p8, p8, p8, p8, p8, None, ref) == -1


def _small(oracle, n_kf=8, n_lm=80, obs=30):
    s = synth.ba_sequence(n_kf, n_lm, obs)
    nL = len(s["points_gt"])
    pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                   torch.from_numpy(s["meas"]), n_kf, nL)
    st = ba_pack.build_structure(pk)
    pri = (np.array([0], np.int32), s["poses_init"][:1], s["prior_sigmas"][None])
    return s, pk, st, pri


def test_reference_lm_in_the_gaussian_limit_is_the_oracle_lm(oracle):
    """Huber with k = 1e12 (every w = 1, rho = d^2 / 2) walks the oracle's Gaussian LM: validates the reference."""
    s, pk, st, pri = _small(oracle)
    P = oracle.BAProblem(pk, s["K"], s["sigma"], pri)
    oposes, opoints, orep = oracle.ba_lm_optimize(P, st["band"], s["poses_init"], s["points_init"])
    R = robust_ref.RobustBA(oracle, pk, s["K"], s["sigma"], 1, 1e12, pri)
    lin, olin = R.linearize(s["poses_init"], s["points_init"]), oracle.ba_linearize(P, s["poses_init"], s["points_init"])
    for key in ("W", "V", "gl", "Hpp", "gp"):
        assert np.abs(lin[key] - olin[key]).max() <= 1e-11 * np.abs(olin[key]).max(), key
    assert lin["err"] == pytest.approx(olin["err"], rel=1e-12) and np.all(lin["w"] == 1.0)
    assert R.error(s["poses_init"], s["points_init"]) == pytest.approx(oracle.ba_error(P, s["poses_init"], s["points_init"]),
                                                                        rel=1e-12)
    poses, points, rep = R.lm(s["poses_init"], s["points_init"])
    assert (rep["outer"], rep["tries"], rep["status"], rep["iterations"]) == \
        (orep["outer"], orep["tries"], orep["status"], orep["iterations"])
    assert np.allclose(rep["lambda_hist"], orep["lambda_hist"], rtol=1e-12, atol=0)
    assert rep["final_error"] == pytest.approx(orep["final_error"], rel=1e-9)
    assert np.abs(poses - oposes).max() <= 1e-9 * np.abs(oposes).max()
    assert np.abs(points - opoints).max() <= 1e-8 * np.abs(opoints).max()


def test_reference_robust_linearisation_is_consistent(oracle):
    """0.5 sum w d^2 is the linear error at delta = 0; with outliers it is below the Gaussian error and differs from
    sum rho; the reweighted system's gradient is sum w J^T b."""
    s, pk, st, pri = _small(oracle)
    synth.inject_outliers(s, 0.1, seed=7)
    pk = ba_pack.pack_observations(torch.from_numpy(s["obs_pose"]), torch.from_numpy(s["obs_point"]),
                                   torch.from_numpy(s["meas"]), 8, len(s["points_gt"]))
    R = robust_ref.RobustBA(oracle, pk, s["K"], s["sigma"], 2, 3.0, pri)
    lin = R.linearize(s["poses_init"], s["points_init"])
    assert R.linear_error(np.zeros((8, 6)), np.zeros((R.nL, 3))) == pytest.approx(lin["err"], rel=1e-14)
    assert lin["w"].min() < 0.01 and lin["err"] != pytest.approx(R.error(s["poses_init"], s["points_init"]), rel=1e-3)
