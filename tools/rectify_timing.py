"""Time vus_rectify_remap on a resident stereo stream with the test rig's radtan maps (tests/rectify_ref.py): HIP event
pairs around each launch, one warm-up round, the median of the runs.  Two yardsticks are timed in the same process,
alternating with the kernel:

  copy    torch.Tensor.copy_ of the same [frames, 2, H, W] uint8 tensor: the traffic floor (every byte read once and
          written once);
  direct  the same kernel with an all-zero `boxes` array, so that every tile gathers its four neighbours from global
          memory instead of staging its source box in LDS (w = 0 is how the plan marks such a tile: no switch is needed).

The numbers go into profiles/rectify.md next to the parent's fast_detect stage time (python bench.py).

    python tools/rectify_timing.py [--frames 1000] [--runs 10] [--height 720] [--width 1280]

Run it under a time limit of its own (`timeout -k 10 600 python tools/rectify_timing.py`)."""
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

import rectify_ref as R                                                                  # noqa: E402
from visual_underwater_slam_amd import _lib, rectify, synth                              # noqa: E402
from visual_underwater_slam_amd.frontend import default_camera                           # noqa: E402

HBM_ACHIEVABLE = 6.29e12      # bytes / s a streaming copy reaches on an MI355X


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    a = ap.parse_args()
    H, W, F = a.height, a.width, a.frames
    assert a.runs >= 3 and F >= 1
    dev = torch.device("cuda:0")
    rig = R.Rig("radtan", H, W)
    rect = rectify.StereoRectifier.from_kalibr(rig.kalibr(), (H, W), new_camera=default_camera(H, W))
    cv = synth.canvas(torch, dev)
    raw = torch.empty((F, 2, H, W), dtype=torch.uint8, device=dev)
    for s in range(0, F, 8):
        n = min(8, F - s)
        raw[s:s + n] = synth.stereo_frames(s, n, H, W, xp=torch, device=dev, canvas_arr=cv)
    out, out_direct, out_copy = torch.empty_like(raw), torch.empty_like(raw), torch.empty_like(raw)
    no_boxes = torch.zeros_like(rect.boxes)
    st = _lib.current_stream_ptr()

    def remap(boxes, dst):
        _lib.call("vus_rectify_remap", _lib.ptr(raw), 2 * F, H, W, W, _lib.ptr(rect.maps), _lib.ptr(boxes), 2, _lib.ptr(dst), W, st)

    variants = {"staged": lambda: remap(rect.boxes, out), "copy": lambda: out_copy.copy_(raw),
                "direct": lambda: remap(no_boxes, out_direct)}
    times = {k: [] for k in variants}
    for it in range(a.runs + 1):                       # round 0 is the warm-up
        for k, fn in variants.items():
            t = timed(fn)
            if it > 0:
                times[k].append(t)
    plan_ms = timed(lambda: _lib.call("vus_rectify_plan", _lib.ptr(rect.maps), 2, H, W, _lib.ptr(rect.boxes), st))
    # faster and different is not faster: both paths against the numpy statement on the first and the last frame
    assert torch.equal(out, out_direct), "staged and direct paths differ"
    for f in (0, F - 1):
        want = R.remap(raw[f].cpu().numpy(), rect.maps_host)
        assert np.array_equal(out[f].cpu().numpy(), want), f"frame {f} differs from the reference"
    boxes = rect.boxes.cpu().numpy()
    bytes_moved = 2 * raw.numel()                      # every image byte read once and written once
    res = {"kernel": "rectify_remap", "frames": F, "H": H, "W": W, "runs": a.runs, "plan_ms": round(plan_ms, 4),
           "tiles_staged": int((boxes[..., 2] > 0).sum()), "tiles": int(boxes[..., 2].size),
           "box_bytes_max": int((((boxes[..., 2] + 6) & ~3) * boxes[..., 3]).max()),
           "displacement_px_max": round(float(np.abs(np.stack(R.unpack_words(rect.maps_host))).max()) / 32, 1),
           "bytes_per_frame": bytes_moved // F, "map_bytes": int(rect.maps.numel() * 4)}
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                  "GBps": round(bytes_moved / med / 1e6, 1), "hbm_share": round(bytes_moved / (med * 1e-3) / HBM_ACHIEVABLE, 3)}
    res["staged_over_copy"] = round(res["staged"]["ms_median"] / res["copy"]["ms_median"], 3)
    res["direct_over_staged"] = round(res["direct"]["ms_median"] / res["staged"]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
