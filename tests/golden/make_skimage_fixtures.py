#!/usr/bin/env python3
"""Generate tests/golden/skimage_fast_orb.npz: scikit-image's FAST-9 corner masks and intensity-centroid orientations
on one synthetic stereo frame, the independent pin of tests/test_thirdparty_crosscheck.py.

    python tests/golden/make_skimage_fixtures.py PYTHON       # PYTHON: an interpreter with scikit-image and numpy

scikit-image is not a dependency of this project, so it runs in that separate interpreter; this script only builds the
input image and stores what scikit-image returned.  Fixtures are data only: the input and scikit-image's outputs.

Stored per threshold t (THRESHOLDS): `mask_t<t>` = corner_fast(img / 255, n=9, (t + 0.5) / 255) > 0, bit-packed over the
flattened (2, H, W) mask; `ang_t<t>` = corner_orientations(img / 255, ., OFAST_MASK) at every corner of that mask inside
the detector border (BORDER <= row < H - BORDER, same for columns), in raster order (image, row, column)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_underwater_slam_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "skimage_fast_orb.npz")
H, W, T0 = 240, 320, 5
THRESHOLDS = (10, 25)
BORDER = 31

_SCRIPT = r'''
import json, sys, numpy as np, skimage
from skimage.feature import corner_fast, corner_orientations
from skimage.feature.orb import OFAST_MASK
img = np.load(sys.argv[1]); thrs = json.loads(sys.argv[2]); B = int(sys.argv[3]); out = sys.argv[4]
f = img.astype(np.float64) / 255.0
res = {"version": np.array(skimage.__version__)}
for thr in thrs:
    masks = np.stack([corner_fast(f[n], 9, (thr + 0.5) / 255.0) > 0 for n in range(f.shape[0])])
    inner = np.zeros_like(masks)
    inner[:, B:-B, B:-B] = masks[:, B:-B, B:-B]
    ang = [corner_orientations(f[n], np.argwhere(inner[n]), OFAST_MASK) for n in range(f.shape[0])]
    res["mask_t%d" % thr] = masks
    res["ang_t%d" % thr] = np.concatenate(ang)
np.savez(out, **res)
'''


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    img = synth.stereo_frames(T0, 1, H=H, W=W)[0]                    # 2 images
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "img.npy"), img)
        script = os.path.join(d, "sk.py")
        with open(script, "w") as fh:
            fh.write(_SCRIPT)
        subprocess.run([sys.argv[1], script, os.path.join(d, "img.npy"), json.dumps(list(THRESHOLDS)), str(BORDER),
                        os.path.join(d, "out.npz")], check=True, env={"PATH": os.environ.get("PATH", "")})
        sk = np.load(os.path.join(d, "out.npz"))
        out = {"img": img, "border": np.int32(BORDER), "thresholds": np.array(THRESHOLDS, np.int32),
               "skimage_version": sk["version"]}
        for thr in THRESHOLDS:
            out[f"mask_t{thr}"] = np.packbits(sk[f"mask_t{thr}"].ravel())
            out[f"ang_t{thr}"] = sk[f"ang_t{thr}"]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
