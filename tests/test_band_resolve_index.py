"""Every address vus_ba_band_resolve forms inside the stored factor, swept on the CPU, and its panel recursion replayed on
the CPU through the same address functions against a dense solve (no GPU).

visual-underwater-slam_amd/csrc/band_index.h holds the arithmetic as __host__ __device__ functions (rs_*); resolve_kernel
of band_resolve.hip calls them, and tests/native/band_resolve_check.cpp replays them for every (sweep, panel, chunk, MFMA
step, lane) of the launch: as a library built with UBSan here, and once as a stand-alone program built with
AddressSanitizer + UBSan, reading a real buffer of the band's size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import closure_ref as cr
import marginals_ref as mr
from test_band_index import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "band_resolve_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bandres") / "libbandres_check.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-shared", "-fPIC", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", out])
    lib = ctypes.CDLL(out)
    lib.bandres_sweep.restype = ctypes.c_longlong
    lib.bandres_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_char_p]
    lib.bandres_replay.restype = None
    lib.bandres_replay.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return lib


@pytest.mark.parametrize("n,band", SHAPES)
def test_every_resolve_address_lies_inside_the_factor(checker, n, band):
    """In range, the element the kernel means, and every stored element of the factor read exactly once per sweep."""
    touched = ctypes.c_longlong(0)
    msg = ctypes.create_string_buffer(256)
    bad = checker.bandres_sweep(n, band, ctypes.byref(touched), msg)
    assert bad == 0, msg.value.decode()
    assert touched.value > 0


def test_sweep_as_a_stand_alone_program_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "band_resolve_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    args = [str(v) for shape in SHAPES for v in shape]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(" 0 violations") == len(SHAPES)


@pytest.mark.parametrize("n,band", cr.RESOLVE_SHAPES)
def test_the_recursion_solves_the_dense_system(checker, n, band):
    """The factor laid out as the one-sided band solve leaves it (closure_ref.stored_factor: NaN wherever nothing is
    stored), the kernel's recursion on the CPU: the dense solution to round-off."""
    rng = np.random.default_rng(1000 * n + band)
    A, _ = mr.random_spd_band(rng, n, band)
    L = cr.stored_factor(A, band)
    B = rng.normal(size=(3, 6 * n))
    X = B.copy()
    checker.bandres_replay(L.ctypes.data, n, band, X.ctypes.data, 3)
    ref = np.linalg.solve(A, B.T).T
    assert np.isfinite(X).all()
    assert np.abs(X - ref).max() <= 1e-13 * np.abs(ref).max()
