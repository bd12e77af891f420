"""Compile-only check of the tiled orientation + rBRIEF kernel's resources (no GPU needed).

orient_rbrief_kernel<*, *, true> waits on patch gathers for most of its time and hides that latency with more waves, so
its occupancy is part of its speed: 7 waves per SIMD need <= 72 VGPRs (AGPRs included), <= 160 KiB / 7 bytes of LDS per
256-thread workgroup and no scratch.  This test compiles orient.hip for gfx950 with the Makefile's own flags and reads
the compiler's resource report, so that a later change cannot lower the occupancy unnoticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-underwater-slam_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

WAVES = 7
MAX_VGPRS = 72                        # allocation granule 8: 512 / 7 -> 72
MAX_LDS = 160 * 1024 // WAVES         # one workgroup = one wave per SIMD


def _make_var(name):
    return subprocess.check_output(["make", "-s", "-C", CSRC, name], text=True).strip()


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("orient_res") / "orient.co"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", *_make_var("print-offload").split(), "-Wno-unused-function",
           *_make_var("print-frontend-flags").split(), "--cuda-device-only", "-c", os.path.join(CSRC, "orient.hip"),
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


def _tiled_instances(kernels):
    # orient_rbrief_kernel<EXACT, ORDERED, TILED>: mangled ...orient_rbrief_kernelILb?ELb?ELb1EE...
    found = {k: v for k, v in kernels.items() if re.search(r"orient_rbrief_kernelILb[01]ELb[01]ELb1E", k)}
    assert len(found) == 2, sorted(kernels)
    return found


def test_tiled_orient_registers(resources):
    for name, r in _tiled_instances(resources).items():
        assert r["VGPRs"] + r["AGPRs"] <= MAX_VGPRS, (name, r)


def test_tiled_orient_lds(resources):
    for name, r in _tiled_instances(resources).items():
        assert r["LDS Size"] <= MAX_LDS, (name, r)


def test_tiled_orient_no_scratch(resources):
    for name, r in _tiled_instances(resources).items():
        assert r["ScratchSize"] == 0, (name, r)


def test_tiled_orient_occupancy(resources):
    for name, r in _tiled_instances(resources).items():
        assert r["Occupancy"] >= WAVES, (name, r)
