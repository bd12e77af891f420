"""include/vus_fixed_lag_nav.h: the header stands alone, its symbols are declared there only, exported and bound, every
invalid argument is refused on the host before any launch, and the host classes refuse what the family does not serve (no
GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vus_fixed_lag_nav.h")
SYMBOLS = {"vus_nav_window_prior_check": 3, "vus_nav_window_prior_linearize": 8, "vus_nav_window_prior_assemble": 6,
           "vus_nav_window_prior_eval_step": 11, "vus_nav_window_prior_error": 7, "vus_nav_window_prior_compact": 6}


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_is_self_contained_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "vus_fixed_lag_nav.h"\nint main(void) { vus_nav_window_prior p; p.m = 1; return p.m - 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_symbols_are_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = _strip(open(HDR).read())
    own = _strip(open(os.path.join(ROOT, "include", "vus.h")).read())
    assert '#include "vus_fixed_lag_nav.h"' in own
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert name not in own                       # declared in its own header only
        assert hasattr(lib, name)
        assert len(L.ADDENDA_SIGNATURES[name]) == n_args and name not in L.SIGNATURES
        assert getattr(L.load(), name).restype is ctypes.c_int
    name = "vus_nav_window_prior_work_doubles"
    assert re.search(r"\blong long\s+" + name + r"\s*\(", hdr) and name not in own and hasattr(lib, name)
    assert getattr(L.load(), name).restype is ctypes.c_longlong
    assert L.load().vus_abi_version() == 1
    from visual_underwater_slam_amd.ba import _CNavWindowPrior
    assert [f for f, _ in _CNavWindowPrior._fields_] == ["n_poses", "first", "m", "x0", "v0", "b0", "H", "g", "c"]


def test_the_header_is_an_addendum_with_the_c_compilers_layout(tmp_path):
    """The reader keeps the ABI in two parts: abi(), whose size tests/test_abi_reader.py pins, and addenda(), where this header
    is read; the binding takes both.  sizeof and every offsetof of the new struct as gcc sees the header."""
    from visual_underwater_slam_amd import _abi
    add, core = _abi.addenda(), _abi.abi()
    assert "vus_fixed_lag_nav.h" in _abi.ADDENDA
    assert sorted(add.functions) == sorted(list(SYMBOLS) + ["vus_nav_window_prior_work_doubles"])
    assert list(add.structs) == ["vus_nav_window_prior"] and add.constants == {}
    assert not set(add.functions) & set(core.functions) and not set(add.structs) & set(core.structs)
    both = _abi.whole()
    assert len(both.functions) == len(core.functions) + 7 and len(both.structs) == len(core.structs) + 1
    assert both.constants == core.constants
    name, fields = "vus_nav_window_prior", add.structs["vus_nav_window_prior"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vus_fixed_lag_nav.h"', "int main(void) {",
             f'  printf("{name} %zu\\n", sizeof({name}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({name}, {f}));' for f, _ in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    cls = _abi.struct(name)
    assert ctypes.sizeof(cls) == int(c[name])
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == int(c[f]), f


def _prior(n_poses=10, first=2, m=3, x0=8, v0=8, b0=8, H=8, g=8, c=0.0):
    from visual_underwater_slam_amd.ba import _CNavWindowPrior
    return _CNavWindowPrior(n_poses, first, m, x0, v0, b0, H, g, c)


def test_arguments_are_refused_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                          # never dereferenced: every call below fails validation first

    def refused(fn, *args, word):
        rc = getattr(lib, fn)(*args, None)
        assert rc == -1 and word in lib.vus_last_error(), (fn, lib.vus_last_error())
    bads = [(_prior(m=0), b"m=0"), (_prior(m=-2), b"m=-2"), (_prior(m=1366, n_poses=5000), b"m=1366"),
            (_prior(first=8), b"exceeds n_poses"), (_prior(first=-1), b"first=-1"), (_prior(n_poses=0), b"n_poses"),
            (_prior(first=0, m=11), b"exceeds n_poses")]
    bads += [(_prior(**{a: None}), b"null") for a in ("x0", "v0", "b0", "H", "g")]
    for bad, word in bads:
        a = ctypes.byref(bad)
        refused("vus_nav_window_prior_check", a, 12, word=word)
        refused("vus_nav_window_prior_linearize", a, *[p8] * 6, word=word)
        refused("vus_nav_window_prior_assemble", a, p8, 12, p8, p8, word=word)
        refused("vus_nav_window_prior_eval_step", a, *[p8] * 9, word=word)
        refused("vus_nav_window_prior_error", a, *[p8] * 5, word=word)
    good = ctypes.byref(_prior())
    refused("vus_nav_window_prior_check", None, 12, word=b"null")
    refused("vus_nav_window_prior_check", good, 7, word=b"3 m - 1 = 8 exceeds the band of 7 nodes")
    refused("vus_nav_window_prior_check", good, -1, word=b"band")
    refused("vus_nav_window_prior_check", ctypes.byref(_prior(c=float("nan"))), 8, word=b"not finite")
    refused("vus_nav_window_prior_assemble", good, p8, 7, p8, p8, word=b"exceeds the band")
    for fn, n_ptr in (("vus_nav_window_prior_linearize", 6), ("vus_nav_window_prior_eval_step", 9), ("vus_nav_window_prior_error", 5)):
        for k in range(n_ptr):
            args = [p8] * n_ptr
            args[k] = None
            refused(fn, good, *args, word=b"null")
    for k in (0, 2, 3):
        a2 = [p8, 8, p8, p8]
        a2[k] = None
        refused("vus_nav_window_prior_assemble", good, *a2, word=b"null")
    for w, word in ((0, b"w=0"), (-1, b"w=-1"), (1366, b"w=1366")):
        refused("vus_nav_window_prior_compact", p8, p8, w, p8, p8, word=word)
    for k in (0, 1, 3, 4):
        a3 = [p8, p8, 2, p8, p8]
        a3[k] = None
        refused("vus_nav_window_prior_compact", *a3, word=b"null")
    assert lib.vus_nav_window_prior_work_doubles(good) == 4 * 45 + 2 * 1 + 8
    assert lib.vus_nav_window_prior_work_doubles(None) == 0
    assert lib.vus_nav_window_prior_work_doubles(ctypes.byref(_prior(m=0))) == 0


def _arrays(m):
    x0 = np.tile(np.r_[np.eye(3).reshape(-1), 0.0, 0.0, 0.0], (m, 1))
    return x0, np.zeros((m, 3)), np.zeros((m, 6))


def test_nav_window_prior_shapes_and_fits():
    from visual_underwater_slam_amd import ba

    class Problem:
        pose_stride, n_poses, band = 3, 10, 9
    x0, v0, b0 = _arrays(3)
    I, z = np.eye(45), np.zeros(45)
    with pytest.raises(ValueError, match="outside"):
        ba.NavWindowPrior(8, x0, v0, b0, I, z, 0.0, 10, device="cpu")
    with pytest.raises(ValueError, match=r"\[45, 45\]"):
        ba.NavWindowPrior(2, x0, v0, b0, np.eye(18), z, 0.0, 10, device="cpu")
    with pytest.raises(ValueError, match=r"\[45, 45\]"):
        ba.NavWindowPrior(2, x0, v0, b0, I, np.zeros(18), 0.0, 10, device="cpu")
    with pytest.raises(ValueError, match=r"\[3, 3\] and \[3, 6\]"):
        ba.NavWindowPrior(2, x0, v0[:2], b0, I, z, 0.0, 10, device="cpu")
    with pytest.raises(ValueError, match=r"\[3, 3\] and \[3, 6\]"):
        ba.NavWindowPrior(2, x0, v0, b0[:1], I, z, 0.0, 10, device="cpu")
    W = ba.NavWindowPrior(2, x0, v0, b0, I, z, 0.0, 10, device="cpu")
    assert (W.first, W.m, W.span, W.pose_stride, W.n) == (2, 3, 2, 3, 1)
    P8 = type("P8", (Problem,), {"band": 8})
    W._fits(P8)                                      # 3 m - 1 = 8 nodes: B of the last keyframe against X of the first
    for field, value, word in (("pose_stride", 1, "pose_stride 3 only"), ("pose_stride", 2, "pose_stride 3 only"),
                               ("n_poses", 11, "the problem has 11 poses"), ("band", 7, "between_span=3")):
        P = type("P", (Problem,), {field: value})
        with pytest.raises(ValueError, match=word):
            W._fits(P)


def test_the_solvers_refuse_what_they_do_not_serve():
    from visual_underwater_slam_amd import ba, dist

    class Problem:
        pose_stride, n_poses, band = 3, 10, 9
    x0, v0, b0 = _arrays(3)
    W = ba.NavWindowPrior(2, x0, v0, b0, np.eye(45), np.zeros(45), 0.0, 10, device="cpu")
    with pytest.raises(NotImplementedError, match="NavWindowPrior.*NavBASolver"):
        ba.NavBASolver(Problem, None, window_prior=W)
    with pytest.raises(NotImplementedError, match="NavWindowPrior"):
        dist.ShardedStereoBASolver(None, None, None, 10, 0, None, 1.0, window_prior=W)
    # the pose-only prior stays refused by both inertial solvers, by its name, before anything else
    Wp = ba.WindowPrior(2, x0, np.eye(18), np.zeros(18), 0.0, 10, device="cpu")
    for cls in (ba.NavBASolver, ba.NavBiasBASolver):
        with pytest.raises(NotImplementedError, match=r"ba\.WindowPrior"):
            cls(Problem, None, window_prior=Wp)
    with pytest.raises(ValueError, match="pose_stride 1 only"):
        Wp._fits(Problem)
