"""include/vus_fixed_lag.h: the header stands alone, its symbols are declared there only, exported and bound, and every
invalid argument is refused on the host before any launch (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vus_fixed_lag.h")
SYMBOLS = {"vus_window_prior_check": 3, "vus_window_prior_linearize": 6, "vus_window_prior_assemble": 6,
           "vus_window_prior_eval_step": 7, "vus_window_prior_error": 5, "vus_ba_band_marginalize": 11}
SIZES = ("vus_window_prior_work_doubles", "vus_ba_band_marginalize_work_doubles")


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_is_self_contained_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "vus_fixed_lag.h"\nint main(void) { vus_window_prior p; p.m = 1; return p.m - 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_symbols_are_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = _strip(open(HDR).read())
    own = _strip(open(os.path.join(ROOT, "include", "vus.h")).read())
    assert '#include "vus_fixed_lag.h"' in own
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert name not in own                       # declared in its own header only
        assert hasattr(lib, name)
        assert len(L.SIGNATURES[name]) == n_args
        assert getattr(L.load(), name).restype is ctypes.c_int
    for name in SIZES:
        assert re.search(r"\blong long\s+" + name + r"\s*\(", hdr) and name not in own and hasattr(lib, name)
        assert getattr(L.load(), name).restype is ctypes.c_longlong
    assert L.load().vus_abi_version() == 1


def _prior(n_poses=10, first=2, m=3, x0=8, H=8, g=8, c=0.0):
    from visual_underwater_slam_amd.ba import _CWindowPrior
    return _CWindowPrior(n_poses, first, m, x0, H, g, c)


def test_window_prior_arguments_are_refused_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                          # never dereferenced: every call below fails validation first

    def refused(fn, *args, word):
        rc = getattr(lib, fn)(*args, None)
        assert rc == -1 and word in lib.vus_last_error(), (fn, lib.vus_last_error())
    bads = ((_prior(m=0), b"m=0"), (_prior(m=-2), b"m=-2"), (_prior(first=8), b"exceeds n_poses"), (_prior(first=-1), b"first=-1"),
            (_prior(n_poses=0), b"n_poses"), (_prior(first=0, m=11), b"exceeds n_poses"), (_prior(x0=None), b"null"),
            (_prior(H=None), b"null"), (_prior(g=None), b"null"))
    for bad, word in bads:
        a = ctypes.byref(bad)
        refused("vus_window_prior_check", a, 4, word=word)
        refused("vus_window_prior_linearize", a, p8, p8, p8, p8, word=word)
        refused("vus_window_prior_assemble", a, p8, 4, p8, p8, word=word)
        refused("vus_window_prior_eval_step", a, p8, p8, p8, p8, p8, word=word)
        refused("vus_window_prior_error", a, p8, p8, p8, word=word)
    good = ctypes.byref(_prior())
    refused("vus_window_prior_check", None, 4, word=b"null")
    refused("vus_window_prior_check", good, 1, word=b"exceeds the band")          # m - 1 = 2 > band
    refused("vus_window_prior_check", good, -1, word=b"band")
    refused("vus_window_prior_check", ctypes.byref(_prior(c=float("nan"))), 4, word=b"not finite")
    refused("vus_window_prior_assemble", good, p8, 1, p8, p8, word=b"exceeds the band")
    for k in range(4):
        args = [p8] * 4
        args[k] = None
        refused("vus_window_prior_linearize", good, *args, word=b"null")
    for k in range(5):
        args = [p8] * 5
        args[k] = None
        refused("vus_window_prior_eval_step", good, *args, word=b"null")
    for k in range(3):
        args = [p8] * 3
        args[k] = None
        refused("vus_window_prior_error", good, *args, word=b"null")
        a2 = [p8, 4, p8, p8]
        a2[(0, 2, 3)[k]] = None
        refused("vus_window_prior_assemble", good, *a2, word=b"null")
    assert lib.vus_window_prior_work_doubles(good) == 24 * 3 + 2 * 1 + 8
    assert lib.vus_window_prior_work_doubles(None) == 0 and lib.vus_window_prior_work_doubles(ctypes.byref(_prior(m=0))) == 0


def test_band_marginalize_arguments_are_refused_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)
    good = dict(S=p8, n=12, band=9, gs=p8, k=3, H=p8, g=p8, quad=p8, status=p8, work=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_ba_band_marginalize(a["S"], a["n"], a["band"], a["gs"], a["k"], a["H"], a["g"], a["quad"], a["status"],
                                         a["work"], None)
        return rc, lib.vus_last_error()
    cases = [(dict(n=1), b"n_nodes"), (dict(n=0), b"n_nodes"), (dict(n=5000), b"n_nodes"), (dict(band=-1), b"band="),
             (dict(band=12), b"band="), (dict(k=0), b"n_drop"), (dict(k=-1), b"n_drop"), (dict(k=12), b"n_drop"),
             (dict(k=13), b"n_drop"), (dict(k=1), b"wider than band + 1"), (dict(band=7), b"wider than band + 1")]
    cases += [({name: None}, b"null") for name in ("S", "gs", "H", "g", "quad", "status", "work")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    ld = 16 * ((6 * 12 + 1 + 15) // 16)
    assert lib.vus_ba_band_marginalize_work_doubles(12, 9, 3) == ld * ld
    assert lib.vus_ba_band_marginalize_work_doubles(12, 9, 2) == ld * ld            # a tail of exactly band + 1 nodes
    for bad in ((12, 9, 1), (12, 9, 0), (12, 9, 12), (1, 0, 1), (12, 12, 3)):
        assert lib.vus_ba_band_marginalize_work_doubles(*bad) == 0


def test_the_host_classes_refuse_what_the_family_does_not_serve():
    import numpy as np
    from visual_underwater_slam_amd import ba

    class Problem:
        pose_stride, n_poses, band = 1, 10, 4
    x0 = np.tile(np.r_[np.eye(3).reshape(-1), 0.0, 0.0, 0.0], (3, 1))
    with pytest.raises(ValueError, match="outside"):
        ba.WindowPrior(8, x0, np.eye(18), np.zeros(18), 0.0, 10, device="cpu")
    with pytest.raises(ValueError, match=r"\[18, 18\]"):
        ba.WindowPrior(2, x0, np.eye(12), np.zeros(18), 0.0, 10, device="cpu")
    W = ba.WindowPrior(2, x0, np.eye(18), np.zeros(18), 0.0, 10, device="cpu")
    assert (W.first, W.m, W.span) == (2, 3, 2)
    W._fits(Problem)
    for field, value, word in (("pose_stride", 2, "pose_stride 1 only"), ("n_poses", 11, "the problem has 11 poses"),
                               ("band", 1, "between_span=WindowPrior.span")):
        P = type("P", (Problem,), {field: value})
        with pytest.raises(ValueError, match=word):
            W._fits(P)
    # the inertial solvers and the sharded solver refuse the family by name, before anything else
    from visual_underwater_slam_amd import dist
    for cls, args in ((ba.NavBASolver, (Problem, None)), (ba.NavBiasBASolver, (Problem, None))):
        with pytest.raises(NotImplementedError, match="WindowPrior"):
            cls(*args, window_prior=W)
    with pytest.raises(NotImplementedError, match="WindowPrior"):
        dist.ShardedStereoBASolver(None, None, None, 10, 0, None, 1.0, window_prior=W)
