"""Compile-only check of the FAST tile kernels' resources (no GPU needed).

The tile kernels are bound by vector-instruction issue and hide their LDS latency with eight waves per SIMD: that needs
<= 64 VGPRs, <= 20,480 B of LDS per 256-thread workgroup (eight workgroups per CU) and no scratch.  This test compiles
detect.hip for gfx950 with the Makefile's own flags and reads the compiler's resource report, so that a later change
cannot lower the occupancy unnoticed.  The persistent retry kernel (no work in a normal step) is held to no scratch
and to the seven waves (72 VGPRs) it has."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-underwater-slam_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

WAVES = 8
MAX_VGPRS = 64                        # 512 / 8
MAX_LDS = 160 * 1024 // WAVES         # 20,480 B: one workgroup = one wave per SIMD


def _make_var(name):
    return subprocess.check_output(["make", "-s", "-C", CSRC, name], text=True).strip()


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("fast_res") / "detect.co"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", *_make_var("print-offload").split(), "-Wno-unused-function",
           *_make_var("print-frontend-flags").split(), "--cuda-device-only", "-c", os.path.join(CSRC, "detect.hip"),
           "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def _instances(kernels, pattern, count):
    found = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(found) == count, (pattern, sorted(kernels))
    return found


def _all_fast(kernels):
    # fast_tile_kernel<WRITE_SCORE, DETECT, BLUR, REGIONS> (five instances), fast_tile_tiled_kernel<REGIONS> (two),
    # fast_sample_kernel, fast_retry_kernel
    return {**_instances(kernels, r"\d+fast_tile_kernelILb", 5), **_instances(kernels, r"\d+fast_tile_tiled_kernelILb", 2),
            **_instances(kernels, r"\d+fast_sample_kernelE", 1), **_instances(kernels, r"\d+fast_retry_kernelE", 1)}


def _detection_and_sample(kernels):
    return {k: v for k, v in _all_fast(kernels).items() if "fast_retry_kernel" not in k}


def test_fast_no_scratch(resources):
    for name, r in _all_fast(resources).items():
        assert r["ScratchSize"] == 0, (name, r)


def test_fast_registers(resources):
    for name, r in _detection_and_sample(resources).items():
        assert r["VGPRs"] + r["AGPRs"] <= MAX_VGPRS, (name, r)


def test_fast_lds(resources):
    for name, r in _detection_and_sample(resources).items():
        assert r["LDS Size"] <= MAX_LDS, (name, r)


def test_fast_occupancy(resources):
    for name, r in _detection_and_sample(resources).items():
        assert r["Occupancy"] >= WAVES, (name, r)


def test_fast_retry_keeps_seven_waves(resources):
    for name, r in _instances(resources, r"\d+fast_retry_kernelE", 1).items():
        assert r["VGPRs"] + r["AGPRs"] <= 72 and r["Occupancy"] >= 7, (name, r)     # 512 / 7 -> 72
