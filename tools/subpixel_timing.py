"""vus_stereo_refine timing on the MI355X at the shape of BASELINE.json configs[1] (1280 x 720, 2000 keypoint slots), next to
the hamming_stereo stage it follows: the front end processes F synthetic stereo frames (synth.stereo_frames), then each of
the two entry points is launched --batch times back to back between two device events, on the front end's own tables; the
figure is the median over --reps of (elapsed / batch), after a warm-up.  Window and search sizes from the smallest to the
largest, the default (5, 5) first; and (5, 5) once more on tables whose matched slots were moved to the front of every list,
which is what a compaction pass in front of the kernel would buy.  Writes one JSON line.

    python tools/subpixel_timing.py [--reps 15] [--batch 50] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visual_underwater_slam_amd import _lib, synth  # noqa: E402
from visual_underwater_slam_amd.frontend import ImageProcessorParams, StereoOrbFrontend  # noqa: E402

H, W, K = 720, 1280, 2000


def per_call_us(fn, reps, batch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ts.append(1e3 * a.elapsed_time(b) / batch)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "max_kp": K, "reps": a.reps, "batch": a.batch, "frames": {}}
    ptr = _lib.ptr
    for F in (1, 8, 32):
        img = torch.from_numpy(synth.stereo_frames(0, F, H=H, W=W)).cuda()
        fe = StereoOrbFrontend(H, W, max_frames=F, params=ImageProcessorParams(max_features=K))
        r = fe.process(img)
        torch.cuda.synchronize()
        p, st = fe.p, _lib.current_stream_ptr()
        idx, dist = torch.empty_like(r.stereo_idx), torch.empty_like(r.stereo_dist)

        def hamming():
            _lib.call("vus_hamming_match", ptr(r.desc), ptr(r.kp_keys), ptr(r.kp_count), K, H, W, ptr(fe.stereo_q), ptr(fe.stereo_t),
                      F, p.stereo_threshold, p.min_disparity, p.max_disparity, p.stereo_max_distance, ptr(idx), ptr(dist), st)

        row = {"matches": int((r.stereo_idx >= 0).sum().item()), "hamming_stereo_us": per_call_us(hamming, a.reps, a.batch)}
        assert torch.equal(idx, r.stereo_idx)
        disp = torch.empty((F, K), dtype=torch.int32, device="cuda")
        stat = torch.empty((F, K), dtype=torch.uint8, device="cuda")
        for hw, sr in ((5, 5), (1, 1), (3, 8), (7, 8)):
            def refine():
                _lib.call("vus_stereo_refine", ptr(img), F, H, W, W, ptr(r.stereo_idx), ptr(r.kp_keys), ptr(r.kp_count), K, hw, sr,
                          ptr(disp), ptr(stat), st)
            row[f"refine_hw{hw}_s{sr}_us"] = per_call_us(refine, a.reps, a.batch)
        # would compacting the matched slots first pay?  The same matches moved to the front of every left list (count =
        # the number of matches), so that whole workgroups hold matched slots only and the others leave on the count
        sidx, keys, cnt = r.stereo_idx.clone(), r.kp_keys.clone(), r.kp_count.clone()
        order = torch.argsort((sidx < 0).to(torch.int8), dim=1, stable=True)
        sidx = torch.gather(sidx, 1, order).contiguous()
        keys[0::2] = torch.gather(keys[0::2], 1, order)
        cnt[0::2] = (sidx >= 0).sum(1).to(torch.int32)

        def compacted():
            _lib.call("vus_stereo_refine", ptr(img), F, H, W, W, ptr(sidx), ptr(keys), ptr(cnt), K, 5, 5, ptr(disp), ptr(stat), st)
        row["refine_hw5_s5_compacted_tables_us"] = per_call_us(compacted, a.reps, a.batch)
        _, status = fe.refine_stereo(r, img)
        row["status_counts_ok_edge_none"] = [int((status == v).sum().item()) for v in (0, 1, 255)]
        res["frames"][str(F)] = row
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
