"""vus_stereo_pair_pose (include/vus_loop.h) is exported and bound, and refuses every invalid argument on the host, before
any launch, with a message that names it (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "vus_loop.h")).read()
    assert re.search(r"\bint\s+vus_stereo_pair_pose\s*\(", hdr)
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vus.h")).read(), flags=re.S)
    assert '#include "vus_loop.h"' in own and "vus_stereo_pair_pose" not in own      # declared in its own header only
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "vus_stereo_pair_pose")
    assert len(L.SIGNATURES["vus_stereo_pair_pose"]) == 22
    n_args = len(re.search(r"vus_stereo_pair_pose\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S).group(1).split(","))
    assert n_args == 22
    assert L.load().vus_stereo_pair_pose.restype is ctypes.c_int


def test_invalid_arguments_are_rejected_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                       # never dereferenced: every call below fails validation first
    cam = np.array([609.0, 609.2, 322.97, 187.1, 0.063])
    good = dict(match=p8, pa=p8, pb=p8, stereo=p8, keys=p8, count=p8, F=4, P=2, K=2000, H=360, W=640, cam=cam.ctypes.data,
                thr=2.0, hyp=256, seed=1, refine=10, T=p8, JtJ=p8, rss=p8, out=p8, info=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_stereo_pair_pose(a["match"], a["pa"], a["pb"], a["stereo"], a["keys"], a["count"], a["F"], a["P"], a["K"],
                                      a["H"], a["W"], a["cam"], a["thr"], a["hyp"], a["seed"], a["refine"], a["T"], a["JtJ"],
                                      a["rss"], a["out"], a["info"], None)
        return rc, lib.vus_last_error()

    for name in ("match", "pa", "pb", "stereo", "keys", "count", "cam", "T", "JtJ", "rss", "out", "info"):
        rc, msg = call(**{name: None})
        assert rc == -1 and b"null" in msg, name
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(P=0), b"n_pairs"), (dict(P=-3), b"n_pairs"), (dict(F=0), b"n_frames"), (dict(F=-1), b"n_frames"),
                     (dict(K=0), b"max_kp"), (dict(K=4097), b"max_kp"), (dict(K=8192), b"max_kp"),
                     (dict(hyp=0), b"n_hyp"), (dict(hyp=4097), b"n_hyp"), (dict(refine=-1), b"refine_iters"),
                     (dict(refine=65), b"refine_iters"), (dict(H=0), b"H="), (dict(W=0), b"W="),
                     (dict(thr=0.0), b"threshold_px"), (dict(thr=-2.0), b"threshold_px"), (dict(thr=nan), b"threshold_px"),
                     (dict(thr=inf), b"threshold_px")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for bad in (0.0, -1.0, nan, inf):
        for slot, word in ((0, b"focal"), (1, b"focal"), (4, b"baseline")):
            c = cam.copy()
            c[slot] = bad
            rc, msg = call(cam=c.ctypes.data)
            assert rc == -1 and word in msg, (bad, slot, msg)
    assert lib.vus_abi_version() == 1
