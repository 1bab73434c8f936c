#!/usr/bin/env python3
"""Pin the packed 4:2:2 conversion spec (tests/_yuv422_spec.py) against a REAL OpenCV: run wherever `import cv2` works.

    python tests/golden/make_yuv422_goldens_with_cv2.py

Writes tests/golden/yuv422_cv2_probe.npz (~200 KB): two frames of shape (H, W, 2) and what cv2.cvtColor makes of them through BOTH codes,
cv2.COLOR_YUV2BGR_YUY2 and cv2.COLOR_YUV2BGR_UYVY (the same bytes read in either order) --
  * `corners`: every Y value 0 .. 255 against every (U, V) pair of the chroma corner cases below, laid out as YUYV (one row per pair; the
    UYVY reading of the same bytes swaps the roles, which is as good a probe);
  * `random`: uniformly random bytes, 64 x 48 texels;
and the OpenCV version.  tests/test_yuv422_cv2_probe.py compares the spec with it and skips while the file is absent.  Commit the .npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("BEVW_YUV422_PROBE_OUT", os.path.join(HERE, "yuv422_cv2_probe.npz"))
CORNERS = (0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255)


def corner_frame() -> np.ndarray:
    """(169, 256, 2) as YUYV: row j holds Y = 0 .. 255 against the j-th (U, V) pair."""
    pairs = [(u, v) for u in CORNERS for v in CORNERS]
    f = np.empty((len(pairs), 256, 2), np.uint8)
    f[..., 0] = np.arange(256, dtype=np.uint8)
    for j, (u, v) in enumerate(pairs):
        f[j, 0::2, 1], f[j, 1::2, 1] = u, v
    return f


def main():
    import cv2

    if "shim" in getattr(cv2, "__file__", "") or not hasattr(cv2, "COLOR_YUV2BGR_YUY2"):
        raise SystemExit("this is not a real OpenCV")
    rng = np.random.default_rng(13)
    frames = {"corners": corner_frame(), "random": rng.integers(0, 256, (48, 64, 2), dtype=np.uint8)}
    out = {"cv2_version": np.array(cv2.__version__)}
    for k, f in frames.items():
        out[k + "_yuv422"] = f
        out[k + "_bgr_yuyv"] = cv2.cvtColor(f, cv2.COLOR_YUV2BGR_YUY2)
        out[k + "_bgr_uyvy"] = cv2.cvtColor(f, cv2.COLOR_YUV2BGR_UYVY)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "OpenCV", cv2.__version__, "%d bytes" % os.path.getsize(OUT))


if __name__ == "__main__":
    sys.exit(main())
