"""Worker of tests/test_gray_gpu.py::test_plan_switched_off: one fresh process, because the library reads BEVW_REMAP_PLAN once.

argv: case_file.  The parent sets BEVW_REMAP_PLAN=0 in this process's environment and leaves grey frames and the expected images
(oracle.remap on the 2-D arrays) in case_file; the maps are `minify8` of the catalogue (tests/_caller_maps.py), which is deterministic.
The one-channel remapper must serve the step with k_remap_lut_gray (BEVW_PATH_PER_PIXEL) at tolerance 0."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _caller_maps as CM  # noqa: E402
from tests import _harness as H  # noqa: E402


def main():
    case_file = sys.argv[1]
    ffi, _ = H.worker_library({"BEVW_REMAP_PLAN": "0"})
    z = np.load(case_file)
    frames, want = z["frames"], z["want"]
    size = CM.SMALL
    maps = CM.family("minify8", *size)
    outside = H.outside_of(maps[0], size[0], size[1])
    with H.Remapper(ffi, maps, size, channels=1) as g:
        got = g.remap(frames)
        assert g.last_path() == ffi.PATH_PER_PIXEL, g.last_path()
    for b in range(frames.shape[0]):
        H.assert_same_gray(got[b], want[b], outside, "plan off, image %d" % b)
    print("worker OK", flush=True)


if __name__ == "__main__":
    main()
