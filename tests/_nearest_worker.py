"""Worker of tests/test_nearest_gpu.py::test_plan_switches_off: one fresh process, because the library reads BEVW_PLAN_UNITS and
BEVW_REMAP_PLAN once.

argv: the switch's name.  The parent sets <switch>=0 in this process's environment.  The maps are `minify8` of the catalogue
(tests/_caller_maps.py) and the frames are seeded, so nothing travels but the name.  A nearest remapper must serve the step with k_remap_nn8 /
k_remap_nn16 (BEVW_PATH_PER_PIXEL) at tolerance 0 against the NumPy statement, at both depths, label frames and full-range frames."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _caller_maps as CM  # noqa: E402
from tests import _harness as H  # noqa: E402
from tests import _nearest as NN  # noqa: E402


def main():
    switch = sys.argv[1]
    assert switch in ("BEVW_PLAN_UNITS", "BEVW_REMAP_PLAN")
    ffi, _ = H.worker_library({switch: "0"})
    size = CM.SMALL
    sw, sh = size[:2]
    m1, m2 = CM.family("minify8", *size)
    outside = ~NN.inside_nn(m1, m2, sw, sh)
    assert outside.any()
    with H.Remapper(ffi, (m1, m2), size, channels=1) as g:
        NN.set_interpolation(g, True)
        for depth in (8, 16, 8):
            NN.set_depth(g, depth)
            for make in (NN.label_frames, NN.random_frames):
                frames = make(sw, sh, 3, 2900, depth)
                got = NN.remap_nn(g, frames)
                assert g.last_path() == ffi.PATH_PER_PIXEL, g.last_path()
                NN.assert_batch_nn(got, NN.want_nn(frames, m1, m2), outside, "%s=0, %d bits" % (switch, depth))
    print("worker OK", flush=True)


if __name__ == "__main__":
    main()
