"""Fixtures in general position (tests/golden/general_position_*.npz, made by tests/golden/make_general_position.py from
a 60-digit mpmath reference): loading, the per-block check, and the f64 CPU twins' outputs for the same cases.  Test
infrastructure only (a plain module, not a conftest); no mpmath here."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_names():
    return sorted(os.path.basename(p)[len("general_position_"):-len(".npz")]
                  for p in glob.glob(os.path.join(GOLDEN, "general_position_*.npz")))


def load_case(name):
    with np.load(os.path.join(GOLDEN, f"general_position_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def outputs(c):
    return [k[5:] for k in c if k.startswith("want_")]


def check_blocks(got, c, keys=None, who=""):
    """max |got - want| <= tol_block for every block of every array in keys; prints the worst ratio per array first."""
    r = ratios(got, c, keys)
    for k in r:
        print(f"{who} {k:10s} worst error / tol_block = {r[k]:.3g}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{who}: blocks outside their bound (worst error / tol_block): {bad}"
    return r


def oracle_outputs(O, c):
    """The outputs of a case by the f64 CPU twins, keyed like its want_ arrays."""
    return proj_oracle_outputs(O, c) if "obs_pose" in c else nav_oracle_outputs(O, c) if "imu_pim" in c else pose_oracle_outputs(O, c)


def nav_oracle_outputs(O, c):
    """vus_nav_linearize_cpu / vus_nav_eval_step_cpu on an inertial case."""
    import nav_ref
    nP = len(c["poses"])
    N = O.NavFactors(c["gravity"][0], imu=(c["imu_i"], c["imu_j"], c["imu_pim"], c["imu_W"]),
                     dvl=(c["dvl_pose"], c["dvl_meas"], c["dvl_sigma"][:, 0]), vprior=(c["vp_idx"], c["vp_v"], c["vp_sigma"]))
    assert np.array_equal(N.dvl_w, c["dvl_w"][:, 0]) and np.array_equal(N.vp_w, c["vp_w"])
    lin = nav_ref.nav_linearize(O, N, c["poses"], c["vels"], c["bias"][0])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    nv, nb, out = np.zeros((nP, 3)), np.zeros(6), np.zeros(2)
    rc = O.lib().vus_nav_eval_step_cpu(N.ref(), nP, O._p(f(c["poses"])), O._p(f(c["vels"])), O._p(f(c["bias"][0])), O._p(f(c["dc"])),
                                       O._p(f(c["db"][0])), O._p(f(c["new_poses"])), O._p(nv), O._p(nb), O._p(out), None)
    assert rc == 0
    return {"Snav": lin["Snav"].reshape(-1, 36), "Scb": lin["Scb"], "Sbb": lin["Sbb"][None], "gnav": lin["gnav"], "gb": lin["gb"][None],
            "nav_err": np.array([[lin["err"]]]), "new_vels": nv, "new_bias": nb[None], "nav_eval": out.reshape(2, 1)}


def proj_oracle_outputs(O, c):
    """point_prior_ref.PointPriorBA (the oracle's stereo factor, mono_ref's pinhole factor, sensor_ref's extrinsic, robust_ref's
    table and aggregation) on a projection case, once per loss kind."""
    import point_prior_ref
    pk = {"n_poses": len(c["poses"]), "n_points": len(c["points"]), "n_obs": len(c["obs_pose"]), "obs_pose": c["obs_pose"],
          "obs_point": c["obs_point"], "meas": c["meas"]}
    S = c["sensor"][0] if len(c["sensor"]) else None
    out = {}
    for kind, k in zip(c["loss_kind"].tolist(), c["loss_k"][:, 0].tolist()):
        ba = point_prior_ref.PointPriorBA(O, pk, c["K"][0], float(c["sigma"][0, 0]), kind, k, S, c["is_mono"], c["mono_K"][0],
                                          float(c["mono_sigma"][0, 0]), point_priors=(c["pp_idx"], c["pp_mean"], c["pp_sigma"]))
        assert ba.w_sig == c["inv_sigma"][0, 0] and ba.mono_w == c["mono_w"][0, 0] and np.array_equal(ba.pp_w, c["pp_w"])
        lin = ba.linearize(c["poses"], c["points"])
        npo, npt = ba.retract(c["poses"], c["points"], c["dp"], c["dl"])
        e_lin, e_new = ba.observation_errors(c["poses"], c["points"], c["dp"], c["dl"])
        for name, v in (("W", lin["W"]), ("weights", lin["w"][:, None]), ("V", lin["V"]), ("gl", lin["gl"]), ("Hpp", lin["Hpp"]),
                        ("gp", lin["gp"]), ("err", [[lin["obs_err"]]]), ("eval", [[e_lin], [e_new]]),
                        ("error", [[ba.error(c["poses"], c["points"]) - ba.prior_error(c["points"])]])):
            out[f"{name}_k{kind}"] = np.asarray(v, np.float64)
        out.update(new_poses=npo, new_points=npt, pp_err=np.array([[lin["pp_err"]]]),
                   pp_eval=np.array([[ba.prior_error(c["points"] + c["dl"])], [ba.prior_error(npt)]]))
    return out


def pose_oracle_outputs(O, c):
    """A pose case by the oracle's pose_local / pose_retract under between_ref's numpy."""
    import between_ref as br
    G = br.BetweenSet(c["btw_i"], c["btw_j"], c["btw_meas"], c["btw_sigma"], list(zip(c["btw_kind"].tolist(), c["btw_k"].tolist())))
    assert np.array_equal(G.w, c["btw_w"])
    poses, dp, nP = c["poses"], c["dp"], len(c["poses"])
    fac = br.factors(O, G, poses)
    lin = np.zeros((len(fac), 120))
    for f, (rw, J1, J2, a, b, _, _) in enumerate(fac):
        lin[f] = np.concatenate([(J1.T @ J1).reshape(-1), (J1.T @ J2).reshape(-1), (J2.T @ J2).reshape(-1), J1.T @ rw, J2.T @ rw])
    out = {"btw_lin": lin, "btw_err": np.array([[sum(0.5 * float(f[0] @ f[0]) for f in fac)]]),
           "btw_eval": np.array([[br.linear_error(fac, dp.reshape(-1))], [br.error(O, G, c["btw_new_poses"])]])}
    pri = (c["prior_pose"], c["prior_T"], c["prior_w"])
    H, g, e = br.prior_system(O, pri, poses)
    out["Hpp"] = np.stack([H[6 * i:6 * i + 6, 6 * i:6 * i + 6].reshape(-1) for i in range(nP)])
    out["gp"], out["err"] = g.reshape(nP, 6), np.array([[e]])
    new = np.stack([O.pose_retract(poses[i], dp[i]) for i in range(nP)])
    x = dp.reshape(-1)
    out["new_poses"] = new
    out["eval"] = np.array([[e + float(g @ x) + 0.5 * float(x @ H @ x)], [br.prior_error(O, pri, new)]])
    return out


def ratios(got, c, keys=None):
    """Worst |got - want| / tol_block per output array."""
    out = {}
    for k in keys or outputs(c):
        diff, tol = np.abs(got[k] - c["want_" + k]).max(axis=1), c["tol_" + k].astype(np.float64)
        out[k] = float(np.where(diff == 0.0, 0.0, diff / np.where(tol > 0.0, tol, np.finfo(float).tiny)).max())    # 0 / 0: exact
    return out
