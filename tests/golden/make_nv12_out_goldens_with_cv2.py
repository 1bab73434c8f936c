#!/usr/bin/env python3
"""Pin the NV12 OUTPUT spec (tests/_nv12_out_spec.py) against a REAL OpenCV: run wherever `import cv2` works.

    python tests/golden/make_nv12_out_goldens_with_cv2.py

Writes tests/golden/nv12_out_cv2_probe.npz (~100 KB): BGR images and what cv2.cvtColor(img, cv2.COLOR_BGR2YUV_I420) makes of them --
  * `blocks`: 2 x 2 blocks of four different colours (random), so that the chroma of a block's top-left pixel and the block average differ
    -- it tells which of the two OpenCV takes;
  * `ramps`: every value 0 .. 255 of each channel alone and of grey, against the other channels at the corner values below, one pixel per
    2 x 2 block (the block's four pixels equal): it pins the rounding of Y, U and V over every value, with nothing to average;
and the OpenCV version.  tests/test_nv12_out_cv2_probe.py compares the spec with it and skips while the file is absent.  Commit the .npz.
(If a real cv2 averages the blocks, the NV12 output's chroma needs whole 2 x 2 blocks per writer, and the plan compiler would have to cut
units on even rows and columns: DESIGN.md section 8.)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("BEVW_NV12_OUT_PROBE_OUT", os.path.join(HERE, "nv12_out_cv2_probe.npz"))
CORNERS = (0, 1, 127, 128, 254, 255)


def blocks_image() -> np.ndarray:
    """64 x 96 BGR: every 2 x 2 block four random, pairwise different colours."""
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    img[1::2, 1::2] = 255 - img[0::2, 0::2]   # the bottom-right pixel far from the top-left one
    return img


def ramps_image() -> np.ndarray:
    """BGR rows of 2 x 2 blocks of one colour each: per (channel or grey, corner value of the other channels) one block row of 256 values."""
    rows = []
    for ch in range(4):                      # B, G, R alone, then grey
        for other in CORNERS:
            px = np.full((256, 3), other, np.uint8)
            v = np.arange(256, dtype=np.uint8)
            if ch == 3:
                px[:] = v[:, None]
            else:
                px[:, ch] = v
            rows.append(np.repeat(np.repeat(px[None], 2, axis=0), 2, axis=1))   # (2, 512, 3)
            if ch == 3:
                break
    return np.concatenate(rows)


def main():
    import cv2

    if "shim" in getattr(cv2, "__file__", "") or not hasattr(cv2, "COLOR_BGR2YUV_I420"):
        raise SystemExit("this is not a real OpenCV")
    out = {"cv2_version": np.array(cv2.__version__)}
    for k, img in (("blocks", blocks_image()), ("ramps", ramps_image())):
        out[k + "_bgr"] = img
        out[k + "_i420"] = cv2.cvtColor(img, cv2.COLOR_BGR2YUV_I420)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "OpenCV", cv2.__version__, "%d bytes" % os.path.getsize(OUT))


if __name__ == "__main__":
    sys.exit(main())
