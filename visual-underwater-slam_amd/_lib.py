"""ctypes binding of libvus_hip.so (C ABI: include/vus.h).  Fails loudly when the library is absent."""
import ctypes
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# VUS_HIP_LIB: another build of the same library (A/B timing of kernel variants); never a different implementation
LIB_PATH = os.environ.get("VUS_HIP_LIB") or os.path.join(_HERE, "csrc", "libvus_hip.so")

# name -> argtypes of every function the headers declare (include/vus.h and the vus_*.h it includes; _abi reads them)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _abi.abi().functions.items()}
# the same for the headers of _abi.ADDENDA (what joined after the size of the table above was pinned); load() binds both and
# what _abi.SUPPLEMENTS names (_abi.full())
ADDENDA_SIGNATURES = {name: argtypes for name, (_, argtypes) in _abi.addenda().functions.items()}

TUNE_BAND_MODE, TUNE_CB_MAX_WG, TUNE_LAST_BAND_MODE, TUNE_WIN_FAULT = (
    _abi.const("VUS_TUNE_" + k) for k in ("BAND_MODE", "CB_MAX_WG", "LAST_BAND_MODE", "WIN_FAULT"))
STATUS_WAIT_EXPIRED, STATUS_WINDOW_EXPIRED = _abi.const("VUS_STATUS_WAIT_EXPIRED"), _abi.const("VUS_STATUS_WINDOW_EXPIRED")


class VusError(RuntimeError):
    """A libvus_hip.so entry point returned a negative code (gtsam raises RuntimeError likewise)."""


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so (soname libamdhip64.so.7).  Import it FIRST so that this
    # library binds to the same HIP runtime instance; loaded the other way round the process ends
    # up with two runtimes and every launch fails with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C visual-underwater-slam_amd/csrc`. There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _abi.full().functions.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise VusError(f"{name} failed ({rc}): {_explain_missing_code_object(lib.vus_last_error().decode())}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def target_mismatch(built: str, device_arch: str):
    """None if code objects built for target ID `built` (e.g. "gfx950:xnack-") load on a device whose gcnArchName is
    `device_arch` (e.g. "gfx950:sramecc+:xnack-"); else the sentence to raise.  A feature the build pins (":xnack-")
    must be the device's setting; a feature it leaves open matches any."""
    b, d = built.split(":"), device_arch.split(":")
    if b[0] != d[0]:
        return (f"libvus_hip.so was built for {built} but the device is {device_arch}: this library targets MI355X "
                f"(gfx950) only")
    for feat in b[1:]:
        if feat not in d[1:]:
            return (f"libvus_hip.so was built for target ID {built} but the device runs {device_arch}: no code object "
                    f"matches (every launch would fail with 'no kernel image is available'). Rebuild with "
                    f"`make -C visual-underwater-slam_amd/csrc clean all OFFLOAD=--offload-arch={b[0]}`")
    return None


def _explain_missing_code_object(text: str) -> str:
    """A launch that fails because no code object of the library matches the device says "no kernel image is available" /
    "invalid device function" and nothing else.  Only THEN is the device's target ID looked up (hipGetDeviceProperties
    costs ~30 ms the first time in a process: measured as 42 -> 75 ms on the first optimize() of a process when it sat in
    require_gpu()) and compared with the one the library was built for."""
    if "no kernel image" not in text and "invalid device function" not in text:
        return text
    try:
        import torch
        arch = getattr(torch.cuda.get_device_properties(torch.cuda.current_device()), "gcnArchName", "")
        why = target_mismatch(load().vus_build_target().decode(), arch) if arch else None
    except Exception:
        why = None
    return f"{text} -- {why}" if why else text


def check_target():
    """Explicit form of the same check (diagnostics, tests): raises if the library's code objects cannot load here."""
    import torch
    arch = getattr(torch.cuda.get_device_properties(torch.cuda.current_device()), "gcnArchName", "")
    why = target_mismatch(load().vus_build_target().decode(), arch) if arch else None
    if why:
        raise RuntimeError(why)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("visual_underwater_slam_amd needs an MI355X (HIP device); no GPU is visible "
                           "and there is deliberately no CPU fallback.")
