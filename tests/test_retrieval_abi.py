"""vus_keyframe_similarity (include/vus_retrieval.h) is declared in its own header, exported and bound, and refuses every
invalid argument on the host, before any launch, with a message that names it (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = 13


def test_symbol_is_declared_exported_and_bound():
    import visual_underwater_slam_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "vus_retrieval.h")).read()
    assert re.search(r"\bint\s+vus_keyframe_similarity\s*\(", hdr)
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vus.h")).read(), flags=re.S)
    assert '#include "vus_retrieval.h"' in own and "vus_keyframe_similarity" not in own   # declared in its own header only
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "vus_keyframe_similarity")
    assert len(L.SIGNATURES["vus_keyframe_similarity"]) == N_ARGS
    decl = re.search(r"vus_keyframe_similarity\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S).group(1)
    assert len(decl.split(",")) == N_ARGS
    assert L.load().vus_keyframe_similarity.restype is ctypes.c_int


def test_invalid_arguments_are_rejected_without_a_gpu():
    import visual_underwater_slam_amd._lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)                       # never dereferenced: every call below fails validation first
    good = dict(desc=p8, kp_count=p8, n_img=20, max_kp=2000, q_img=p8, n_q=10, t_img=p8, n_t=10, t_limit=p8, top=512,
                max_dist=35, S=p8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vus_keyframe_similarity(a["desc"], a["kp_count"], a["n_img"], a["max_kp"], a["q_img"], a["n_q"], a["t_img"],
                                         a["n_t"], a["t_limit"], a["top"], a["max_dist"], a["S"], None)
        return rc, lib.vus_last_error()

    for name in ("desc", "kp_count", "q_img", "t_img", "S"):
        rc, msg = call(**{name: None})
        assert rc == -1 and b"null" in msg and name.encode() in msg, (name, msg)
    for kw, word in ((dict(n_img=0), b"n_img"), (dict(n_img=-2), b"n_img"), (dict(n_q=0), b"n_q"), (dict(n_q=-1), b"n_q"),
                     (dict(n_t=0), b"n_t"), (dict(n_t=-7), b"n_t"),
                     (dict(n_q=65536, n_t=32768), b"n_q * n_t"), (dict(n_q=2**31 - 1, n_t=2), b"n_q * n_t"),
                     (dict(max_kp=0, top=1), b"max_kp"), (dict(max_kp=-5, top=1), b"max_kp"),
                     (dict(max_kp=65536, top=512), b"max_kp"),
                     (dict(top=0), b"top"), (dict(top=-1), b"top"), (dict(top=2001), b"top"), (dict(max_kp=100, top=101), b"top"),
                     (dict(max_dist=-1), b"max_dist"), (dict(max_dist=257), b"max_dist")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # the bounds themselves are accepted by the validation: a null output pointer is then the first complaint
    for kw in (dict(n_q=65536, n_t=32767), dict(n_q=2**31 - 1, n_t=1), dict(max_kp=65535, top=65535), dict(max_kp=1, top=1),
               dict(max_dist=0), dict(max_dist=256), dict(t_limit=None)):
        rc, msg = call(S=None, **kw)
        assert rc == -1 and b"S is null" in msg, (kw, msg)
    assert lib.vus_abi_version() == 1
