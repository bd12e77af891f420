"""visual_underwater_slam_amd._abi, the reader of include/vus*.h behind the Python binding: against the C compiler on the real
headers, and on snippets of every form it must read, skip or refuse (no GPU needed)."""
import ctypes
import os
import subprocess
from ctypes import c_char_p, c_double, c_int, c_longlong, c_ubyte, c_uint32, c_void_p

import pytest

from visual_underwater_slam_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_and_constants_are_the_c_compilers(tmp_path):
    """sizeof and every offsetof of every struct, and the value of every constant, as gcc sees the headers."""
    A = _abi.abi()
    assert len(A.structs) == 11 and "vus_ba_problem" in A.structs and "vus_window_prior" in A.structs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vus.h"', '#include "vus_tiled.h"', "int main(void) {"]
    for name, fields in A.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in fields]
    lines += [f'  printf("{c} %lld\\n", (long long){c});' for c in A.constants]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name in A.structs:
        cls = _abi.struct(name)
        assert ctypes.sizeof(cls) == int(c[name]), name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == int(c[f"{name}.{f}"]), (name, f)
    assert len(A.constants) >= 50
    for name, value in A.constants.items():
        assert value == int(c[name]), name


def test_the_between_struct_keeps_its_layout():
    cls = _abi.struct("vus_between_factors")
    assert cls._fields_[-1] == ("sqrt_info", c_void_p) and len(cls._fields_) == 15
    assert cls.sqrt_info.offset == 104 and ctypes.sizeof(cls) == 112 and cls.tgt_terms.offset == 96


def test_the_headers_are_read_once_and_orb_tables_not_at_all(monkeypatch):
    first = _abi.abi()
    monkeypatch.setattr(_abi, "parse", None)            # a second read would fail
    assert _abi.abi() is first and _abi.const("VUS_ABI_VERSION") == 1
    assert len(first.functions) == 119 and "vus_tiled_offset" not in first.functions
    assert not any("ORB" in k or "BLUR" in k for k in first.constants)


def test_a_missing_include_directory_is_an_import_error_that_names_it(monkeypatch):
    monkeypatch.setattr(_abi, "INCLUDE_DIR", "/nonexistent/include")
    with pytest.raises(ImportError, match="/nonexistent/include"):
        _abi.abi.__wrapped__()


PROTOTYPES = """
#ifdef __cplusplus
extern "C" {
#endif
/* a prototype over three lines, comments between its parameters */
int vus_three_lines(const uint8_t* img,   /* [n_img, H, pitch] */
                    int n_img, int H,     // two on a line
                    uint32_t seed, double thr, int32_t* out, void* stream);
int vus_array_param(const double K[6], double cov[], unsigned char flag, long long n_ids);
long long vus_work_bytes(int n);
const char* vus_text(void);
const char *vus_text2();
int vus_unnamed(int, const double*, long long, void*);
#define VUS_QUAL static inline
VUS_QUAL unsigned vus_inline_helper(int y, int W) {
  const unsigned uy = (unsigned)y;
  if (uy > 3) { return vus_other(uy); }
  return uy * (unsigned)W;
}
static inline int vus_inline_int(int a) { return a; }
int vus_after_the_definitions(int a);
#ifdef __cplusplus
}
#endif
"""


def test_prototypes():
    f = _abi.parse(PROTOTYPES).functions
    assert f == {"vus_three_lines": (c_int, [c_void_p, c_int, c_int, c_uint32, c_double, c_void_p, c_void_p]),
                 "vus_array_param": (c_int, [c_void_p, c_void_p, c_ubyte, c_longlong]),
                 "vus_work_bytes": (c_longlong, [c_int]),
                 "vus_text": (c_char_p, []), "vus_text2": (c_char_p, []),
                 "vus_unnamed": (c_int, [c_int, c_void_p, c_longlong, c_void_p]),
                 "vus_after_the_definitions": (c_int, [c_int])}


def test_structs():
    got = _abi.parse("""
#define VUS_N_ROWS 4
typedef struct vus_thing {
  int n_poses, n_points, n_obs;   /* several declarators */
  const double* K;                /* [6] */
  double gravity[3], scale;
  unsigned char flags[VUS_N_ROWS];
  long long total;
  const int *a, b;
  uint64_t* desc;
} vus_thing;
typedef struct { float x; } vus_untagged;
""").structs
    assert got == {"vus_thing": [("n_poses", c_int), ("n_points", c_int), ("n_obs", c_int), ("K", c_void_p),
                                 ("gravity", c_double * 3), ("scale", c_double), ("flags", c_ubyte * 4), ("total", c_longlong),
                                 ("a", c_void_p), ("b", c_int), ("desc", c_void_p)],
                   "vus_untagged": [("x", ctypes.c_float)]}


def test_constants():
    got = _abi.parse("""
#ifndef VUS_GUARD_H
#define VUS_GUARD_H
#define VUS_DEC 40
#define VUS_HEX 0x00FFu
#define VUS_ALL_ONES 0xFFFFFFFFu   /* a comment */
#define VUS_NEG (-3)
#define VUS_NEG_BARE -1
#define VUS_SHIFT (1 << 22)
#define VUS_SHIFT_BARE 3 << 2
  #  define VUS_INDENTED 7U
#define VUS_FLOAT 1.5
#define VUS_EXPR (VUS_DEC + 1)
#define VUS_TEXT "gfx950"
#define VUS_QUAL static inline
#define VUS_FN(x) 3
#define OTHER_PREFIX 5
#endif
""").constants
    assert got == {"VUS_DEC": 40, "VUS_HEX": 255, "VUS_ALL_ONES": 0xFFFFFFFF, "VUS_NEG": -3, "VUS_NEG_BARE": -1,
                   "VUS_SHIFT": 1 << 22, "VUS_SHIFT_BARE": 12, "VUS_INDENTED": 7}


@pytest.mark.parametrize("text, names", [
    ("int vus_f(int n, size_t bytes);", "size_t bytes"),                              # an unknown scalar type
    ("int vus_f(vus_ba_loss loss, void* stream);", "vus_ba_loss loss"),               # a struct by value
    ("int vus_f(int n, void (*done)(int), void* stream);", "vus_f"),                  # a parameter that cannot be split
    ("double vus_f(int n);", "double vus_f(int n)"),                                  # a return type outside the ABI's three
    ("typedef struct { int n; bool on; } vus_s;", "bool on"),                         # struct members it cannot read
    ("typedef struct { int n : 3; } vus_s;", "int n : 3"),
    ("typedef struct { double x[VUS_UNKNOWN]; } vus_s;", "double x[VUS_UNKNOWN]"),
    ("typedef struct { int n; struct { int a; } in; } vus_s;", "vus_s"),
    ("typedef struct { int (*cb)(int); } vus_s;", "(*cb)(int)"),
])
def test_what_it_cannot_read_it_refuses(text, names):
    with pytest.raises(ValueError) as e:
        _abi.parse(text, where="include/vus_snippet.h")
    assert "include/vus_snippet.h" in str(e.value) and names in str(e.value), str(e.value)
