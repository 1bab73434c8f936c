#!/usr/bin/env python3
"""Pin the nearest-neighbour statement (tests/_nearest.py want_nn) against a REAL OpenCV: run wherever `import cv2` works.

    python tests/golden/make_nearest_goldens_with_cv2.py

Writes tests/golden/nearest_cv2.npz (a few hundred KB): for a handful of caller-map families of tests/_caller_maps.py -- random scatter,
the frame corners, int16 extremes, a strip source at the int16 limit -- and for the two wrap sources (32772 texels along one axis, map1 =
32767 with a delta of 1: the sum stored into a short wraps to -32768), label frames at 8 and at 16 bits, the maps, and what
cv2.remap(frame, map1, map2, cv2.INTER_NEAREST, borderMode=cv2.BORDER_CONSTANT, borderValue=0) makes of them; and the OpenCV version.
tests/test_nearest_cv2_probe.py compares the statement with it and skips while the file is absent.  Commit the .npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.environ.get("BEVW_NEAREST_PROBE_OUT", os.path.join(HERE, "nearest_cv2.npz"))
FAMILIES = ("scatter", "corner", "extremes", "strip_w")
DST = (64, 32)   # dw, dh of every case but the wrap sources


def cases():
    """(key, depth, frame [sh, sw], map1, map2) of every probe, from seeds alone."""
    from tests import _caller_maps as CM
    from tests import _nearest as NN

    for name in FAMILIES:
        sw, sh = CM.sizes(name)[0][:2]
        m1, m2 = CM.family(name, sw, sh, *DST)
        for depth in (8, 16):
            yield "%s_%d" % (name, depth), depth, NN.label_frames(sw, sh, 1, 4000, depth)[0], m1, m2
    for tag, size in zip(("wrap_w", "wrap_h"), NN.WRAP_SIZES):
        m1, m2 = NN.wrap_case(size)
        for depth in (8, 16):
            yield "%s_%d" % (tag, depth), depth, np.maximum(NN.label_frames(size[0], size[1], 1, 4001, depth)[0], 1), m1, m2


def main():
    import cv2

    if "shim" in getattr(cv2, "__file__", "") or not hasattr(cv2, "INTER_NEAREST"):
        raise SystemExit("this is not a real OpenCV")
    out = {"cv2_version": np.array(cv2.__version__), "keys": np.array([c[0] for c in cases()])}
    for key, _, frame, m1, m2 in cases():
        out[key + "_src"], out[key + "_map1"], out[key + "_map2"] = frame, m1, m2
        out[key + "_dst"] = cv2.remap(frame, m1, m2, cv2.INTER_NEAREST, borderMode=cv2.BORDER_CONSTANT, borderValue=0)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "OpenCV", cv2.__version__, "%d bytes" % os.path.getsize(OUT))


if __name__ == "__main__":
    sys.exit(main())
