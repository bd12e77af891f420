#!/usr/bin/env python3
"""Generate tests/golden/between_diag_bits.npz: what the BetweenFactorPose3 kernels (include/vus_between.h, the long
set's vus_closure_linearize included) give for a small set under DIAGONAL models, bit for bit, with the inputs that gave
it.  It was captured on an MI355X from the commit before full-covariance models (vus_between_factors.sqrt_info) went
in; tests/test_between_gauss_gpu.py replays the stored inputs and compares the bits, so that "the diagonal path is
unchanged" is tested and not only asserted.  Regenerate it only from a commit whose diagonal arithmetic is meant to
become the new truth (needs the GPU; run from the repo root: python tests/golden/make_between_diag_fixture.py [OUT]).

The case: 8 poses, pose_stride 1, band 4; 7 odometry factors, then closures (4, 1), (1, 4), (1, 4) (both key orders, two
factors on one pair), (7, 3) and (0, 4); Gaussian odometry, Cauchy / Gaussian / Huber / Welsch / Tukey on the closures;
sigmas spanning 1e-3 .. 1 within one factor.  Stored: lin [n, 120] and the error of vus_between_linearize, Sband / gs of
vus_between_assemble into zeros, the two scalars of vus_between_eval_step, vus_between_error, and rows [n, 78] with the
error of vus_closure_linearize on the same set."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 20261020
N, BAND = 8, 4
PAIRS = [(k - 1, k) for k in range(1, N)] + [(4, 1), (1, 4), (1, 4), (7, 3), (0, 4)]
LOSSES = [(0, 0.0)] * (N - 1) + [(2, 0.5), (0, 0.0), (1, 0.3), (5, 1.0), (3, 2.0)]


def case():
    from visual_underwater_slam_amd.gtsam import Pose3, Rot3
    rng = np.random.default_rng(SEED)
    truth = [Pose3(Rot3.Expmap(0.4 * rng.standard_normal(3)), 3.0 * rng.standard_normal(3)) for _ in range(N)]
    meas = np.stack([truth[a].between(truth[b]).retract(0.02 * rng.standard_normal(6)).flat12() for a, b in PAIRS])
    poses = np.stack([T.retract(0.05 * rng.standard_normal(6)).flat12() for T in truth])
    new_poses = np.stack([T.retract(0.05 * rng.standard_normal(6)).flat12() for T in truth])
    sigmas = 10.0 ** rng.uniform(-3, 0, (len(PAIRS), 6))
    dp = 0.01 * rng.standard_normal((N, 6))
    return dict(i=np.array([p[0] for p in PAIRS], np.int32), j=np.array([p[1] for p in PAIRS], np.int32), meas=meas,
                sigmas=sigmas, loss_kind=np.array([l[0] for l in LOSSES], np.int32),
                loss_k=np.array([l[1] for l in LOSSES]), poses=poses, new_poses=new_poses, dp=dp)


def run(c, **model):
    """The kernels' outputs for the inputs `c` (a dict as stored) as numpy arrays; `model` goes to ba.BetweenFactors."""
    import torch
    from visual_underwater_slam_amd import _lib
    from visual_underwater_slam_amd.ba import BetweenFactors
    losses = list(zip(c["loss_kind"].tolist(), c["loss_k"].tolist()))
    B = BetweenFactors(c["i"], c["j"], c["meas"], c["sigmas"], N, loss=losses, **model)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    poses, new_poses, dp = dev(c["poses"]), dev(c["new_poses"]), dev(c["dp"])
    lin, sc, rows, cerr = z(B.n, 120), z(4), z(B.n, 78), z(1)
    Sb, gs, err = z(N, BAND + 1, 36), z(N, 6), z(1)
    lib = _lib.load()
    work = z(int(max(lib.vus_between_work_doubles(B.addr()), lib.vus_closure_work_doubles(B.addr()))))
    p, st = _lib.ptr, _lib.current_stream_ptr()
    _lib.call("vus_between_check", B.addr(), BAND, st)
    _lib.call("vus_between_linearize", B.addr(), p(poses), p(lin), p(sc), p(work), st)
    _lib.call("vus_between_assemble", B.addr(), p(lin), BAND, p(Sb), p(gs), st)
    _lib.call("vus_between_eval_step", B.addr(), p(poses), p(dp), p(new_poses), p(sc[1:]), p(work), st)
    _lib.call("vus_between_error", B.addr(), p(poses), p(err), p(work), st)
    _lib.call("vus_closure_linearize", B.addr(), p(poses), p(rows), p(cerr), p(work), st)
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()
    return dict(lin=n(lin), lin_err=n(sc[:1]), Sband=n(Sb), gs=n(gs), eval=n(sc[1:3]), error=n(err), rows=n(rows),
                rows_err=n(cerr))


def main():
    c = case()
    out = run(c)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "between_diag_bits.npz")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **c, **{"out_" + k: v for k, v in out.items()})
    print(path, os.path.getsize(path))
    assert all(np.isfinite(v).all() for v in out.values()) and os.path.getsize(path) < 40000


if __name__ == "__main__":
    main()
