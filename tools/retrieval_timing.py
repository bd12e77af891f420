"""vus_keyframe_similarity timing on the MI355X (device events around the timed launch, median of --reps after a warm-up).

  triangle256   256 keyframes, max_kp = top = 512, strict lower triangle (32,640 pairs).  The new call, and on the same
                inputs the only earlier route to the same numbers: ONE vus_hamming_match over those pairs (ungated: the FP4
                matcher) plus a torch count of dist <= max_dist.  The two are timed alternately, their results must agree, and
                the spread of each (min, max over the runs) is reported next to the medians.
  survey2000    2000 keyframes, max_kp = 2000, top = 512, min_gap = 5: one figure, next to the unmeasured estimate of about
                50 ms from the track matcher's rate.  There is no earlier implementation at this size.

One process per case, so that a job script can put each under its own time limit; nothing is retried.  Writes one JSON.

    python tools/retrieval_timing.py --case triangle256|survey2000 [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visual_underwater_slam_amd import _lib  # noqa: E402

MAX_DIST = 35


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def related_images(n_img, K, seed):
    """uint64 [n_img, K, 4]: image i is image i-1 permuted, slot j with j % 41 flipped bits (tests/test_retrieval_gpu.py)."""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 2**63, size=(n_img, K, 4), dtype=np.int64).view(np.uint64) ^ \
        (rng.integers(0, 2, size=(n_img, K, 4), dtype=np.uint64) << np.uint64(63))
    rows = np.arange(K)
    for i in range(1, n_img):
        desc[i] = desc[i - 1, rng.permutation(K)]
        for s in range(40):
            on = rows[(rows % 41) > s]
            bits = rng.integers(0, 256, size=len(on))
            desc[i, on, bits // 64] ^= np.uint64(1) << (bits % 64).astype(np.uint64)
    return desc


def similarity_call(desc, count, img, limit, top, S):
    n_img, K, _ = desc.shape
    n = img.numel()

    def fn():
        _lib.call("vus_keyframe_similarity", desc.data_ptr(), count.data_ptr(), n_img, K, img.data_ptr(), n, img.data_ptr(), n,
                  limit.data_ptr(), top, MAX_DIST, S.data_ptr(), _lib.current_stream_ptr())
    return fn


def triangle256(reps):
    F, K = 256, 512
    desc = torch.from_numpy(related_images(F, K, 51).view(np.int64)).cuda()
    count = torch.full((F,), K, dtype=torch.int32, device="cuda")
    img = torch.arange(F, dtype=torch.int32, device="cuda")
    S = torch.empty((F, F), dtype=torch.int32, device="cuda")
    new = similarity_call(desc, count, img, img.clone(), K, S)           # t_limit[b] = b: a < b
    b, a = np.tril_indices(F, -1)
    P = len(a)
    qi, ti = torch.from_numpy(b.astype(np.int32)).cuda(), torch.from_numpy(a.astype(np.int32)).cuda()
    keys = torch.zeros((F, K), dtype=torch.int32, device="cuda")
    idx = torch.empty((P, K), dtype=torch.int32, device="cuda")
    dist = torch.empty((P, K), dtype=torch.int32, device="cuda")
    out = {}

    def old():
        _lib.call("vus_hamming_match", desc.data_ptr(), keys.data_ptr(), count.data_ptr(), K, 64, 64, qi.data_ptr(), ti.data_ptr(),
                  P, -1, 0, 0, MAX_DIST, idx.data_ptr(), dist.data_ptr(), _lib.current_stream_ptr())
        out["count"] = (dist <= MAX_DIST).sum(1, dtype=torch.int32)

    new(); old()
    torch.cuda.synchronize()
    got = S.cpu().numpy()
    agree = bool(np.array_equal(got[b, a], out["count"].cpu().numpy()) and (np.triu(got) == 0).all())
    t_new, t_old = [], []
    for _ in range(reps):                                                # alternately: the same neighbours on the machine
        t_new.append(timed(new))
        t_old.append(timed(old))
    return {"keyframes": F, "max_kp": K, "top": K, "pairs": P, "results_agree": agree, "score_mean": float(got[b, a].mean()),
            "keyframe_similarity": stats(t_new), "hamming_match_plus_count": stats(t_old),
            "bytes_written_new": 4 * F * F, "bytes_written_old": 8 * P * K}


def survey2000(reps):
    F, K, top, min_gap = 2000, 2000, 512, 5
    g = torch.Generator(device="cuda").manual_seed(52)
    desc = torch.randint(-2**63, 2**63 - 1, (F, K, 4), dtype=torch.int64, device="cuda", generator=g)
    count = torch.full((F,), K, dtype=torch.int32, device="cuda")
    img = torch.arange(F, dtype=torch.int32, device="cuda")
    limit = (img - min_gap + 1).clamp_(min=0).contiguous()
    S = torch.empty((F, F), dtype=torch.int32, device="cuda")
    new = similarity_call(desc, count, img, limit, top, S)
    new()
    torch.cuda.synchronize()
    ts = [timed(new) for _ in range(reps)]
    pairs = int(limit.sum().item())
    r = {"keyframes": F, "max_kp": K, "top": top, "min_gap": min_gap, "pairs": pairs, "distances": pairs * top * top,
         "keyframe_similarity": stats(ts), "estimate_from_the_matcher_rate_ms": 50.0, "score_max": int(S.max().item())}
    r["distances_per_s"] = r["distances"] / (1e-3 * r["keyframe_similarity"]["median_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("triangle256", "survey2000"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "max_dist": MAX_DIST, "case": a.case}
    res.update(triangle256(a.reps) if a.case == "triangle256" else survey2000(a.reps))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
