"""Host-side pieces of bench.py / ba_bench.py that can be exercised without a GPU: the JSON objects the driver
parses must come out well-formed whatever the stage times are."""
import json
import os
import types

import numpy as np
import pytest

import bench
from visual_underwater_slam_amd import ba_bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_usable_cores_is_positive_and_bounded_by_affinity():
    import os
    n = bench.usable_cores()
    assert 1 <= n <= (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count())


def test_ba_roofline_objects_for_configs2_shape():
    prob = types.SimpleNamespace(n_obs=1926616, n_points=48299, n_poses=2000, n_nodes=2000, band=224,
                                 tiles={"n_entries": 1754967}, n_pairs=57452664)
    ms = {"linearize": 0.26, "schur": 1.8, "band_solve": 4.27, "backsub": 0.1, "eval_step": 0.12}
    top, stages = ba_bench.roofline(prob, ms)
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in top
    assert top["stage"] == "band_solve" and top["kernel"] == "chol_syrk_kernel" and 0 < top["frac"] < 1
    assert top["launches_per_solve"] == 2 * 111 + 28            # two-sided: 111 (TRSM, SYRK) pairs + 28 middle panels
    assert stages["linearize"]["algorithmic_bytes"] == 1926616 * 176 + 2000 * 432 + 48299 * 120   # SURVEY 8d formula
    sch = stages["schur"]                                        # the tile-pair GEMM: MFMA-bound, flops as issued
    assert sch["bound"] == "mfma" and sch["flops"] == 2.0 * 48 * 48 * 3 * 1754967 and 0 < sch["frac"] < 1
    assert sch["useful_flops"] < sch["flops"]
    json.dumps({"roofline": top, "stages": stages})
    fl, n = ba_bench.band_factor_flops(2000, 224)
    assert n == 250 and 1.5e10 < fl < 3e10
    # a short trajectory keeps the one-sided solve
    top2, _ = ba_bench.roofline(types.SimpleNamespace(n_obs=5000, n_points=500, n_poses=50, n_nodes=50, band=40,
                                                      tiles={"n_entries": 1200}, n_pairs=40000), ms)
    assert top2["kernel"] == "chol_trsm_update_kernel"


def test_measured_counters_reads_the_committed_pmc_summary():
    traffic, valu, ns = bench.measured_counters("fast_detect", 1000)
    assert traffic and traffic > 2 * 720 * 1280 * 1000 and valu and valu > 1e9 and 1.0 < ns < 2.5
    assert bench.measured_counters("hamming_track", 10)[0] > 0


DUMP_NAMES = ("frames", "kp_count", "cand_count", "kp_keys", "desc", "angle", "stereo_idx", "stereo_dist", "track_idx",
              "track_dist")


def test_dump_outputs_writes_a_seeded_sample_of_the_last_step(tmp_path):
    """bench.dump_outputs on a stand-in FrontendResult (CPU tensors, 100 frames, 6 keypoint slots): a fixed sample of
    DUMP_FRAMES frames, image rows 2f / 2f + 1, float64 with every integer exact, descriptors as 32-bit words, and -1 in
    every slot at or past the image's kp_count."""
    import torch
    F, K = 100, 6
    g = torch.Generator().manual_seed(1)
    res = types.SimpleNamespace(
        n_frames=F, kp_count=torch.randint(0, K + 1, (2 * F,), dtype=torch.int32, generator=g),
        cand_count=torch.randint(0, 1 << 20, (2 * F,), dtype=torch.int32, generator=g),
        kp_keys=torch.randint(-(1 << 31), 1 << 31, (2 * F, K), dtype=torch.int32, generator=g),
        desc=torch.randint(-(1 << 63), (1 << 63) - 1, (2 * F, K, 4), dtype=torch.int64, generator=g),
        angle=torch.randint(0, 30, (2 * F, K), dtype=torch.uint8, generator=g),
        stereo_idx=torch.randint(-1, K, (F, K), dtype=torch.int32, generator=g),
        stereo_dist=torch.randint(0, 257, (F, K), dtype=torch.int32, generator=g),
        track_idx=torch.randint(-1, K, (F - 1, K), dtype=torch.int32, generator=g),
        track_dist=torch.randint(0, 257, (F - 1, K), dtype=torch.int32, generator=g))
    bench.dump_outputs(res, str(tmp_path / "a"))
    bench.dump_outputs(res, str(tmp_path / "b"))
    d = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in DUMP_NAMES}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in DUMP_NAMES)
    assert all(a.dtype == np.float64 for a in d.values())
    for n in DUMP_NAMES:                                                      # the sample does not change between runs
        assert np.array_equal(d[n], np.load(tmp_path / "b" / (n + ".npy"))), n
    f = d["frames"].astype(np.int64)
    assert len(f) == bench.DUMP_FRAMES and (np.diff(f) > 0).all() and 0 <= f[0] and f[-1] < F
    img = np.stack([2 * f, 2 * f + 1], 1).ravel()
    cnt = res.kp_count.numpy()[img]
    valid = np.arange(K)[None, :] < cnt[:, None]
    assert np.array_equal(d["kp_count"], cnt) and np.array_equal(d["cand_count"], res.cand_count.numpy()[img])
    assert np.array_equal(d["kp_keys"], res.kp_keys.numpy()[img])
    words = res.desc.numpy()[img].view(np.uint32)
    assert np.array_equal(d["desc"][valid], words[valid]) and (d["desc"][~valid] == -1).all()
    assert np.array_equal(d["angle"][valid], res.angle.numpy()[img][valid]) and (d["angle"][~valid] == -1).all()
    sv = valid[0::2]
    for n in ("stereo_idx", "stereo_dist"):
        assert np.array_equal(d[n][sv], getattr(res, n).numpy()[f][sv]) and (d[n][~sv] == -1).all()
    t = f < F - 1
    for n in ("track_idx", "track_dist"):
        assert d[n].shape == (t.sum(), K)
        assert np.array_equal(d[n][sv[t]], getattr(res, n).numpy()[f[t]][sv[t]]) and (d[n][~sv[t]] == -1).all()


def test_native_oracle_is_built_outside_the_checkout():
    """The cpu_baseline legs' -march=native C port is built in a temporary directory, not in oracle/ (the checkout
    bench.py runs from need not be writable), and it is what O.lib(native=True) returns afterwards (oracle/ba_port.py).
    A fresh process: the oracle module of this one may already hold a native library."""
    import subprocess
    import sys
    before = sorted(os.listdir(os.path.join(ROOT, "oracle")))
    code = ("import bench; from oracle import oracle as O; lib = bench.native_oracle(); "
            "assert O.lib(native=True) is lib and bench.native_oracle() is lib; lib.vus_oracle_set_threads(1)")
    r = subprocess.run([sys.executable, "-B", "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(ROOT, "oracle"))) == before


def test_full_is_off_by_default_and_pyramid_needs_it():
    """A plain command line runs the headline alone; the legs beyond it (and --pyramid among them) ask for --full."""
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and not a.pyramid and (a.steps, a.warmup) == (3, 1)
    assert bench.parse(["--full"]).full
    assert bench.parse(["--full", "--pyramid"]).pyramid
    with pytest.raises(SystemExit):
        bench.parse(["--pyramid"])


@pytest.mark.gpu
def test_bench_plain_run_prints_only_the_headline(gpu, tmp_path):
    """`python bench.py` without --full: ONE JSON line with the contract's keys and the front-end's roofline, the last
    timed step's outputs under --dump-outputs, and none of the legs that --full adds."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--frames", "24", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "stage_ms", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0
    for k in ("cpu_baseline", "pyramid8", "ba", "ba_sharded"):
        assert k not in j, k
    d = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in DUMP_NAMES}
    assert np.array_equal(d["frames"], np.arange(24)) and (d["kp_count"] == 2000).all()
    assert d["desc"].shape == (48, 2000, 8) and d["track_idx"].shape == (23, 2000)


@pytest.mark.gpu
def test_bench_command_line_contract_on_a_small_stream(gpu, tmp_path):
    """`python bench.py --full` end to end (with a small stream so that it takes seconds): ONE JSON line with the
    contract's keys, the roofline object of the dominant kernel and the BA legs."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--frames", "24", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], capture_output=True,
                       text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    # the last timed step's outputs: all 24 frames (fewer than DUMP_FRAMES), every image at its 2000 keypoints
    d = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in DUMP_NAMES}
    assert all(a.dtype == np.float64 for a in d.values())
    assert np.array_equal(d["frames"], np.arange(24)) and d["kp_count"].shape == (48,) and (d["kp_count"] == 2000).all()
    assert d["desc"].shape == (48, 2000, 8) and d["track_idx"].shape == (23, 2000)
    assert (d["stereo_idx"] >= 0).mean() > 0.1 and (d["track_idx"] >= 0).mean() > 0.1
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["higher_is_better"] is True
    assert j["roofline"]["bound"] in ("hbm", "mfma") and 0 < j["roofline"]["frac"] < 1
    ba = j["ba"]
    assert ba["lm"]["status"] == 0 and ba["value"] > 0 and ba["dropin"]["same_optimum_as_array_path"] is True
    assert ba["roofline"]["bound"] in ("hbm", "mfma")


@pytest.mark.gpu
def test_bench_two_rank_rehearsal_over_gloo_on_the_one_gpu(gpu):
    """The driver's multi-GPU command line -- torch.distributed.run, one rank per GPU, `bench.py --full --gpus N` --
    rehearsed as two ranks on the ONE visible GPU with VUS_BENCH_BACKEND=gloo (RCCL needs one device per rank): the
    frame-sharded front-end with its gather, and the landmark-sharded LM with its reduce / broadcast, produce ONE JSON
    line from rank 0 that carries what an 8-GPU result needs to be interpreted (bytes per trial, per-stage times)."""
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VUS_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--frames", "24", "--ba-sharded-kf", "300"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0 and out["config"]["frames_per_gpu"] == 24
    sh = out["ba_sharded"]
    assert sh["lm"]["status"] == 0 and sh["value"] > 0 and sh["config"]["ranks"] == 2
    assert sh["config"]["reduce_to_rank0_bytes_per_trial"] == 288 * 300 * (sh["config"]["band_blocks"] + 1) + 48 * 300
    assert set(sh["trial_stage_ms_this_rank"]) == {"linearize+allreduce_err", "schur+reduce_to_rank0", "band_solve_rank0+broadcast_step",
                                                   "backsub", "eval_step+allreduce_err"}
