"""include/vus_closure.h: the header stands alone, its symbols are exported and bound, every invalid argument is refused
on the host before any launch (no GPU needed), and the product package does not mention the oracle."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vus_closure.h")
SYMBOLS = {"vus_ba_band_resolve": 8, "vus_closure_check": 3, "vus_closure_linearize": 6, "vus_closure_gradient": 4,
           "vus_closure_scatter": 4, "vus_closure_capacitance": 5, "vus_closure_correct": 8, "vus_closure_diag_max": 4}


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_is_self_contained_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "vus_closure.h"\nint main(void) { return VUS_CLOSURE_MAX_COLS == 384 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_symbols_are_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = _strip(open(HDR).read())
    own = _strip(open(os.path.join(ROOT, "include", "vus.h")).read())
    assert '#include "vus_closure.h"' in own
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert name not in own                       # declared in its own header only
        assert hasattr(lib, name)
        assert len(L.SIGNATURES[name]) == n_args
        assert getattr(L.load(), name).restype is ctypes.c_int


def test_invalid_arguments_are_rejected_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    big = 1 << 40                                   # never dereferenced: every call below fails validation first
    good = dict(L=ctypes.c_void_p(8), n=40, band=7, X=ctypes.c_void_p(big), cols=6, work=None, wd=0)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_ba_band_resolve(a["L"], a["n"], a["band"], a["X"], a["cols"], a["work"], a["wd"], None)
        return rc, lib.vus_last_error()

    for kw, word in ((dict(L=None), b"null"), (dict(X=None), b"null"), (dict(n=0), b"n_nodes"), (dict(n=-4), b"n_nodes"),
                     (dict(band=-1), b"band"), (dict(band=41), b"band"), (dict(cols=0), b"n_cols"), (dict(cols=-6), b"n_cols"),
                     (dict(cols=385), b"n_cols"), (dict(wd=-1), b"work"), (dict(wd=16), b"work"),
                     (dict(X=ctypes.c_void_p(8 + 8 * 100)), b"overlaps"), (dict(L=ctypes.c_void_p(big + 8)), b"overlaps")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)


def test_closure_stages_check_sizes_and_pointers_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    from visual_underwater_slam_amd.ba import _CBetween
    lib = L.load()
    p8 = ctypes.c_void_p(8)

    def factors(n=2, n_nodes=40, stride=1, node1=8):
        return _CBetween(n, n_nodes, stride, node1, 8, 8, 8, 8, 8, 0, None, None, None, None)       # no target CSR needed

    def refused(fn, *args, word):
        rc = getattr(lib, fn)(*args, None)
        assert rc == -1 and word in lib.vus_last_error(), (fn, lib.vus_last_error())
    good = factors()
    for bad, word in ((factors(n=0), b"long closures"), (factors(n=65), b"long closures"), (factors(n_nodes=1), b"bad sizes"),
                      (factors(stride=4), b"bad sizes"), (factors(n_nodes=41, stride=2), b"bad sizes"), (factors(node1=None), b"null")):
        refused("vus_closure_linearize", ctypes.byref(bad), p8, p8, p8, p8, word=word)
        refused("vus_closure_gradient", ctypes.byref(bad), p8, p8, word=word)
        refused("vus_closure_scatter", ctypes.byref(bad), p8, p8, word=word)
        refused("vus_closure_capacitance", ctypes.byref(bad), p8, p8, p8, word=word)
        refused("vus_closure_correct", ctypes.byref(bad), p8, p8, p8, p8, 1, p8, word=word)
        refused("vus_closure_check", ctypes.byref(bad), 3, word=word)
        refused("vus_closure_diag_max", ctypes.byref(bad), p8, p8, word=word)
    refused("vus_closure_linearize", None, p8, p8, p8, p8, word=b"null")
    refused("vus_closure_linearize", ctypes.byref(good), None, p8, p8, p8, word=b"null")
    refused("vus_closure_gradient", ctypes.byref(good), p8, None, word=b"null")
    refused("vus_closure_scatter", ctypes.byref(good), None, p8, word=b"null")
    refused("vus_closure_capacitance", ctypes.byref(good), p8, p8, None, word=b"null")
    refused("vus_closure_correct", ctypes.byref(good), p8, p8, p8, None, 1, p8, word=b"null")
    refused("vus_closure_diag_max", ctypes.byref(good), None, p8, word=b"null")
    refused("vus_closure_diag_max", ctypes.byref(good), p8, None, word=b"null")
    for n_rhs in (0, -1, 9):
        refused("vus_closure_correct", ctypes.byref(good), p8, p8, p8, p8, n_rhs, p8, word=b"n_rhs")
    refused("vus_closure_check", ctypes.byref(good), -1, word=b"band")
    refused("vus_closure_check", ctypes.byref(good), 40, word=b"band")
    assert lib.vus_closure_work_doubles(ctypes.byref(good)) == 6 * 8 * 2 + 8 and lib.vus_closure_work_doubles(None) == 0


def test_more_than_64_long_factors_are_refused_on_the_host():
    import numpy as np
    from visual_underwater_slam_amd.ba import BetweenFactors
    import pytest
    k = 65
    i, j = np.arange(k) % 10, 20 + np.arange(k) % 19
    meas = np.tile(np.r_[np.eye(3).reshape(-1), 0.0, 0.0, 0.0], (k, 1))
    with pytest.raises(ValueError, match="raise max_span.*fewer closures"):
        BetweenFactors(i, j, meas, np.ones((k, 6)), 40, max_span=8, device="cpu")


def test_product_package_does_not_mention_the_oracle():
    pkg = os.path.join(ROOT, "visual-underwater-slam_amd")
    for rel in ("csrc/band_resolve.hip", "csrc/closure.hip", "csrc/between_device.h", "csrc/band_index.h"):
        assert "oracle" not in open(os.path.join(pkg, rel)).read().lower(), rel
    assert "oracle" not in open(HDR).read().lower()
