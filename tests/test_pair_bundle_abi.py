"""vus_stereo_pair_bundle (include/vus_pair_bundle.h) is declared in a header that stands alone, exported and bound, and
refuses every invalid argument on the host, before any launch, with a message that names it (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = 26


def test_header_stands_alone(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "vus_pair_bundle.h"\nint main(void) { return VUS_LOOP_MAX_REFINE > 0 ? 0 : 1; }\n')
    for cc, std in (("cc", "-std=c11"), ("c++", "-std=c++17")):
        cmd = [cc, std, "-Wall", "-Werror", "-fsyntax-only", "-x", "c" if cc == "cc" else "c++", "-I", os.path.join(ROOT, "include"),
               str(src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_symbol_is_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "vus_pair_bundle.h")).read()
    assert re.search(r"\bint\s+vus_stereo_pair_bundle\s*\(", hdr)
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vus.h")).read(), flags=re.S)
    assert '#include "vus_pair_bundle.h"' in own and "vus_stereo_pair_bundle" not in own     # declared in its own header only
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "vus_stereo_pair_bundle")
    assert len(L.SIGNATURES["vus_stereo_pair_bundle"]) == N_ARGS
    decl = re.search(r"vus_stereo_pair_bundle\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S).group(1)
    assert len(decl.split(",")) == N_ARGS
    assert L.load().vus_stereo_pair_bundle.restype is ctypes.c_int


def test_invalid_arguments_are_rejected_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                       # never dereferenced: every call below fails validation first
    cam = np.array([609.0, 609.2, 322.97, 187.1, 0.063])
    good = dict(match=p8, pa=p8, pb=p8, stereo=p8, keys=p8, count=p8, F=4, P=2, K=2000, H=360, W=640, cam=cam.ctypes.data,
                q8=p8, T_in=p8, info_in=p8, suv=0.5, sd=0.12, gate=4.0, iters=10, T=p8, S=p8, chi2=p8, points=p8, out=p8,
                info=p8)
    order = ("match", "pa", "pb", "stereo", "keys", "count", "F", "P", "K", "H", "W", "cam", "q8", "T_in", "info_in", "suv",
             "sd", "gate", "iters", "T", "S", "chi2", "points", "out", "info")

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_stereo_pair_bundle(*(a[k] for k in order), None)
        return rc, lib.vus_last_error()

    for name in ("match", "pa", "pb", "stereo", "keys", "count", "cam", "T_in", "info_in", "T", "S", "chi2", "points", "out",
                 "info"):
        rc, msg = call(**{name: None})
        assert rc == -1 and b"stereo_pair_bundle" in msg and b"null" in msg, name
    nan, inf = float("nan"), float("inf")
    cases = [(dict(P=0), b"n_pairs"), (dict(P=-3), b"n_pairs"), (dict(F=0), b"n_frames"), (dict(F=-1), b"n_frames"),
             (dict(K=0), b"max_kp"), (dict(K=4097), b"max_kp"), (dict(K=8192), b"max_kp"), (dict(iters=-1), b"iters"),
             (dict(iters=65), b"iters"), (dict(H=0), b"H="), (dict(W=0), b"W=")]
    for bad in (0.0, -1.0, nan, inf, -inf):
        cases += [(dict(suv=bad), b"sigma_uv_px"), (dict(sd=bad), b"sigma_disp_px"), (dict(gate=bad), b"gate")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and b"stereo_pair_bundle" in msg and word in msg, (kw, msg)
    for bad in (0.0, -1.0, nan, inf):
        for slot, word in ((0, b"focal"), (1, b"focal"), (4, b"baseline")):
            c = cam.copy()
            c[slot] = bad
            rc, msg = call(cam=c.ctypes.data)
            assert rc == -1 and word in msg, (bad, slot, msg)
    # a null disp_q8 is the integer-disparity call, not an error: the next refusal is reached
    rc, msg = call(q8=None, gate=0.0)
    assert rc == -1 and b"gate" in msg
    assert lib.vus_abi_version() == 1
