"""The C ABI as ctypes, read from the headers: include/vus.h and every include/vus_*.h (but the generated tables of
vus_orb_tables.h).  One parse per process, on first use.  A declaration this reader cannot read is an error, never a guess.

Three parts.  abi() is the ABI as it stood when its size was pinned (tests/test_abi_reader.py counts its structs and functions);
addenda() is what the headers named in ADDENDA added next, read in the same way, and whole() is both -- pinned in turn by
tests/test_fixed_lag_nav_abi.py; supplements() is what the headers named in SUPPLEMENTS have added since.  full() is all
three, and is what the binding (_lib.py), struct() and const() use.  A new header goes into SUPPLEMENTS and needs nothing
else here -- as long as no test pins the size of full(): the sizes are pinned per UNION today (abi(), then whole()), which
is why there are three parts and not one.  Pinning them per header instead would let the parts fold back into one list."""
import ctypes
import functools
import glob
import os
import re
from collections import namedtuple

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ADDENDA = ("vus_fixed_lag_nav.h",)      # headers that joined after the pinned census, in reading order
# headers that joined after the size of whole() was pinned as well (tests/test_fixed_lag_nav_abi.py counts it): read in the
# same way on top of whole(); full() is everything.  A new header goes HERE and needs nothing else
SUPPLEMENTS = ("vus_combined_imu.h",)

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong,
           "unsigned long long": ctypes.c_ulonglong, "double": ctypes.c_double, "float": ctypes.c_float,
           "char": ctypes.c_char, "unsigned char": ctypes.c_ubyte,
           **{f"{u}int{b}_t": getattr(ctypes, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}

# functions: name -> (restype, [argtypes]);  structs: name -> [(field, ctype)];  constants: name -> int
Abi = namedtuple("Abi", "functions structs constants")

_INT = r"[-+]?\s*(?:0[xX][0-9a-fA-F]+|\d+)[uU]?"
_DEFINE = re.compile(rf"^[ \t]*#[ \t]*define[ \t]+(VUS_\w+)[ \t]+\(?\s*({_INT})\s*(?:<<\s*({_INT})\s*)?\)?[ \t]*$", re.M)
_STRUCT = re.compile(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(.*?)\b(vus_\w+)\s*\(([^()]*)\)", re.S)
_DECLARATOR = re.compile(r"([\w\s*]*?)(\w*)\s*(?:\[\s*(\w*)\s*\])?")


def _int(lit):
    return int(lit.replace(" ", "").rstrip("uU"), 0)


def _ctype(decl, base, constants, fail, member=False):
    """One declarator (`const double* K`, `gravity[3]`, `n_points` after `int n_poses,`) -> (name, ctype, its scalar type).
    `base`: the scalar type of the declarators before it on the line, None for the first or only one.  An array is a pointer
    as a parameter and `ctype * N` as a struct member."""
    if not member and ("*" in decl or "[" in decl):         # most parameters: nothing more to read
        return "", ctypes.c_void_p, None
    bare = " ".join(w for w in decl.split() if w != "const")
    if base is None and bare in SCALARS:                    # `int`: an unnamed parameter
        return "", SCALARS[bare], bare
    m = _DECLARATOR.fullmatch(bare)
    if not m or (member and not m.group(2)):
        fail()
    head, name, dim = m.groups()
    base = " ".join(head.replace("*", " ").split()) or base
    if "*" in head or (dim is not None and not member):
        return name, ctypes.c_void_p, base
    if base not in SCALARS or (dim is not None and not (dim.isdigit() or dim in constants)):
        fail()
    return name, SCALARS[base] if dim is None else SCALARS[base] * (int(dim) if dim.isdigit() else constants[dim]), base


def parse(text, where="<string>", constants=None):
    """The prototypes, structs and integer constants of one header's text.  `constants`: those of the headers read before
    it (an array length may name one)."""
    def refuse(decl):
        def fail():
            raise ValueError(f"{where}: cannot read the declaration `{' '.join(decl.split())}`")
        return fail
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    constants = dict(constants or {})
    for name, a, b in _DEFINE.findall(text):
        constants[name] = _int(a) << _int(b) if b else _int(a)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M).replace('extern "C" {', " ")
    structs = {}
    for body, name in _STRUCT.findall(text):
        fields = structs[name] = []
        for member in filter(str.strip, body.split(";")):
            base = None
            for decl in member.split(","):
                field, ctype, base = _ctype(decl, base, constants, refuse(member), member=True)
                fields.append((field, ctype))
    text = _STRUCT.sub(" ", text)
    while re.search(r"\{[^{}]*\}", text):                   # a function DEFINITION goes, head and body
        text = re.sub(r"[^;{}]*\{[^{}]*\}", " ", text, count=1)
    functions = {}
    for decl in filter(lambda d: d.strip(" \n\t}"), text.split(";")):
        m = _PROTO.fullmatch(decl.strip(" \n\t}"))
        ret = m and " ".join(m.group(1).replace("*", " * ").split()).replace(" *", "*")
        if not m or ret not in RETURNS:
            refuse(decl)()
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        functions[m.group(2)] = (RETURNS[ret], [_ctype(p, None, constants, refuse(decl))[1] for p in params])
    return Abi(functions, structs, constants)


@functools.lru_cache(maxsize=None)
def abi():
    """The pinned part of the ABI (every header but ADDENDA); the headers are read the first time this is called."""
    if not os.path.isdir(INCLUDE_DIR):
        raise ImportError(f"{INCLUDE_DIR} is missing: the Python binding reads the C ABI from the headers there")
    paths = [p for p in sorted(glob.glob(os.path.join(INCLUDE_DIR, "vus*.h"))) if os.path.basename(p) not in ("vus_orb_tables.h",) + ADDENDA + SUPPLEMENTS]
    whole = Abi({}, {}, {})
    for path in paths:                  # vus.h sorts first
        with open(path) as f:
            one = parse(f.read(), path, whole.constants)
        for got, new in zip(whole, one):
            got.update(new)
    return whole


def _read_after(base, names):
    """What the headers `names` declare on top of `base`; a name `base` already holds is an error."""
    new = Abi({}, {}, {})
    for name in names:
        path = os.path.join(INCLUDE_DIR, name)
        known = {**base.constants, **new.constants}
        with open(path) as f:
            one = parse(f.read(), path, known)
        # parse() hands back the constants it was given next to the header's own
        one = one._replace(constants={k: v for k, v in one.constants.items() if k not in known})
        for held, got, more in zip(base, new, one):
            twice = sorted(set(more) & (set(held) | set(got)))
            if twice:
                raise ValueError(f"{path}: {', '.join(twice)} is declared in an earlier header as well")
            got.update(more)
    return new


@functools.lru_cache(maxsize=None)
def addenda():
    """What the headers of ADDENDA declare; a name abi() already holds is an error."""
    return _read_after(abi(), ADDENDA)


@functools.lru_cache(maxsize=None)
def whole():
    """abi() and addenda() together."""
    return Abi(*({**a, **b} for a, b in zip(abi(), addenda())))


@functools.lru_cache(maxsize=None)
def supplements():
    """What the headers of SUPPLEMENTS declare; a name whole() already holds is an error."""
    return _read_after(whole(), SUPPLEMENTS)


@functools.lru_cache(maxsize=None)
def full():
    """whole() and supplements() together: what the library exports and the binding binds."""
    return Abi(*({**a, **b} for a, b in zip(whole(), supplements())))


def const(name):
    return full().constants[name]


def struct(name):
    """A ctypes.Structure class with the layout of the header's `typedef struct { ... } name;`."""
    return type(name, (ctypes.Structure,), {"_fields_": list(full().structs[name])})
