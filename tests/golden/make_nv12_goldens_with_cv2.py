#!/usr/bin/env python3
"""Pin the NV12 conversion spec (tests/_nv12_spec.py) against a REAL OpenCV: run wherever `import cv2` works.

    python tests/golden/make_nv12_goldens_with_cv2.py

Writes tests/golden/nv12_cv2_probe.npz (~250 KB): two NV12 frames and what cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_NV12) makes of them --
  * `corners`: every Y value 0 .. 255 against every (U, V) pair of the chroma corner cases below (one 2 x 2 block per chroma sample, four
    consecutive Y values in it), 128 x 338 texels;
  * `random`: uniformly random bytes, 64 x 48 texels;
and the OpenCV version.  tests/test_nv12_cv2_probe.py compares the spec with it and skips while the file is absent.  Commit the .npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("BEVW_NV12_PROBE_OUT", os.path.join(HERE, "nv12_cv2_probe.npz"))
CORNERS = (0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255)


def corner_frame() -> np.ndarray:
    pairs = [(u, v) for u in CORNERS for v in CORNERS]
    W, H = 128, 2 * len(pairs)                       # 64 blocks per block row hold Y = 0 .. 255; one block row per (U, V) pair
    Y = np.empty((H, W), np.uint8)
    UV = np.empty((H // 2, W), np.uint8)
    for j, (u, v) in enumerate(pairs):
        for i in range(W // 2):
            Y[2 * j:2 * j + 2, 2 * i:2 * i + 2] = np.array([[4 * i, 4 * i + 1], [4 * i + 2, 4 * i + 3]], np.uint8)
        UV[j, 0::2], UV[j, 1::2] = u, v
    return np.concatenate([Y, UV])


def main():
    import cv2

    if "shim" in getattr(cv2, "__file__", "") or not hasattr(cv2, "COLOR_YUV2BGR_NV12"):
        raise SystemExit("this is not a real OpenCV")
    rng = np.random.default_rng(12)
    frames = {"corners": corner_frame(), "random": rng.integers(0, 256, (48 * 3 // 2, 64), dtype=np.uint8)}
    out = {"cv2_version": np.array(cv2.__version__)}
    for k, f in frames.items():
        out[k + "_nv12"] = f
        out[k + "_bgr"] = cv2.cvtColor(f, cv2.COLOR_YUV2BGR_NV12)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "OpenCV", cv2.__version__, "%d bytes" % os.path.getsize(OUT))


if __name__ == "__main__":
    sys.exit(main())
