"""Time vus_clahe_luts and vus_clahe_apply on a resident stereo stream: HIP event pairs around each launch, one warm-up
round, the median of the runs.  Three streams are timed in the same process, alternating:

  textured  synth.stereo_frames, the stream of bench.py (frame standard deviation about 74 grey levels);
  murky     the same frames through the murk model of tests/clahe_ref.py (standard deviation about 3): the lanes of a
            wave add to a handful of histogram bins -- the input CLAHE exists for;
  constant  every pixel 128: all lanes on one bin, the histogram's worst case (black water, a saturated lamp cone).

and one yardstick, `copy`: torch.Tensor.copy_ of the same tensor (every byte read once and written once).  CLAHE's own
traffic floor is 3 bytes per pixel: the table kernel reads the image, the apply kernel reads it again and writes it.

The numbers go into profiles/clahe.md next to the parent's fast_detect stage time (python bench.py).

    python tools/clahe_timing.py [--frames 1000] [--runs 10] [--height 720] [--width 1280] [--tiles 8]

Run it under a time limit of its own (`timeout -k 10 600 python tools/clahe_timing.py`)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clahe_ref as C                                                                    # noqa: E402
from visual_underwater_slam_amd import _lib, clahe, synth                                # noqa: E402

HBM_ACHIEVABLE = 6.29e12      # bytes / s a streaming copy reaches on an MI355X


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def murk_on_device(frames, t0=0.08, s=0.25, A=150.0):
    """clahe_ref.murk in torch float64 (the same operations in the same order), 8 frames at a time."""
    H, W = frames.shape[-2:]
    x = (np.arange(W, dtype=np.float64) - (W - 1) / 2.0) / W
    y = (np.arange(H, dtype=np.float64) - (H - 1) / 2.0) / W
    t = t0 * np.exp(-(x[None, :] ** 2 + y[:, None] ** 2) / (2.0 * s * s))
    td, veil = torch.from_numpy(t).to(frames.device), torch.from_numpy(A * (1.0 - t)).to(frames.device)
    out = torch.empty_like(frames)
    for b in range(0, len(frames), 8):
        out[b:b + 8] = torch.floor(frames[b:b + 8].double() * td + veil + 0.5).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--clip-limit", type=float, default=4.0)
    a = ap.parse_args()
    H, W, F = a.height, a.width, a.frames
    assert a.runs >= 3 and F >= 1
    dev = torch.device("cuda:0")
    en = clahe.Clahe(H, W, tiles=(a.tiles, a.tiles), clip_limit=a.clip_limit)
    cv = synth.canvas(torch, dev)
    textured = torch.empty((F, 2, H, W), dtype=torch.uint8, device=dev)
    for s in range(0, F, 8):
        n = min(8, F - s)
        textured[s:s + n] = synth.stereo_frames(s, n, H, W, xp=torch, device=dev, canvas_arr=cv)
    streams = {"textured": textured, "murky": murk_on_device(textured), "constant": torch.full_like(textured, 128)}
    assert np.array_equal(streams["murky"][0].cpu().numpy(), C.murk(textured[0].cpu().numpy()))
    out = torch.empty_like(textured)
    luts = torch.empty((2 * F, a.tiles, a.tiles, 256), dtype=torch.uint8, device=dev)
    st = _lib.current_stream_ptr()

    def run_luts(src):
        _lib.call("vus_clahe_luts", _lib.ptr(src), 2 * F, H, W, W, a.tiles, a.tiles, en.clip, _lib.ptr(luts), st)

    def run_apply(src):
        _lib.call("vus_clahe_apply", _lib.ptr(src), 2 * F, H, W, W, _lib.ptr(luts), a.tiles, a.tiles, _lib.ptr(out), W, st)

    times = {(k, which): [] for k in streams for which in ("luts", "apply", "copy")}
    for it in range(a.runs + 1):                       # round 0 is the warm-up
        for k, src in streams.items():
            for which, fn in (("luts", run_luts), ("apply", run_apply), ("copy", lambda s_: out.copy_(s_))):
                t = timed(lambda: fn(src))
                if it > 0:
                    times[(k, which)].append(t)
    # faster and different is not faster: both kernels against the numpy statement on the first and the last pair
    for k, src in streams.items():
        run_luts(src)
        run_apply(src)
        torch.cuda.synchronize()
        for f in (0, F - 1):
            pair = src[f].cpu().numpy()
            assert np.array_equal(luts[2 * f:2 * f + 2].cpu().numpy(), C.luts(pair, a.tiles, a.tiles, en.clip)), (k, f)
            assert np.array_equal(out[f].cpu().numpy(), C.clahe(pair, a.tiles, a.tiles, en.clip)), (k, f)
    px = textured.numel()
    res = {"kernel": "clahe", "lib": os.path.basename(_lib.LIB_PATH), "frames": F, "H": H, "W": W, "tiles": a.tiles,
           "clip": en.clip, "runs": a.runs, "std": {k: round(float(v[:4].float().std()), 1) for k, v in streams.items()}}
    for k in streams:
        r = {}
        for which, nbytes in (("luts", px), ("apply", 2 * px), ("copy", 2 * px)):
            t = times[(k, which)]
            med = statistics.median(t)
            r[which] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                        "GBps": round(nbytes / med / 1e6, 1), "hbm_share": round(nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 3)}
        both = r["luts"]["ms_median"] + r["apply"]["ms_median"]
        r["both_ms"] = round(both, 4)
        r["floor_share"] = round(3 * px / (both * 1e-3) / HBM_ACHIEVABLE, 3)      # 3 bytes per pixel at the achievable rate
        res[k] = r
    for k in ("murky", "constant"):
        res[k + "_over_textured"] = {w: round(res[k][w]["ms_median"] / res["textured"][w]["ms_median"], 3) for w in ("luts", "apply")}
        res[k + "_over_textured"]["both"] = round(res[k]["both_ms"] / res["textured"]["both_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
