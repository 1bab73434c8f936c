"""Worker of tests/test_caller_maps_gpu.py::test_plan_switched_off: one fresh process, because the library reads BEVW_REMAP_PLAN once.

argv: case_file.  The parent sets BEVW_REMAP_PLAN=0 in this process's environment and leaves the input frames and the expected BGR images
(oracle.remap on the specification's BGR frames) in case_file; the maps come from the catalogue (tests/_caller_maps.py), which is
deterministic.  Every family at its first size x (BGR, NV12, YUYV frames) x (BGR, NV12 images) runs on k_remap_lut and is compared with
tolerance 0.  Any refusal by the library ends the worker with its error: none of these combinations is refused."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _caller_maps as CM  # noqa: E402
from tests import _harness as H  # noqa: E402
from tests import _nv12_out_spec as SO  # noqa: E402


def main():
    case_file = sys.argv[1]
    ffi, _ = H.worker_library({"BEVW_REMAP_PLAN": "0"})
    z = np.load(case_file)
    cases = CM.child_cases()
    for name, size, inp in cases:
        raw, want = z["raw_%d_%d_%s" % (size[0], size[1], inp)], z["want_%s_%s" % (name, inp)]
        with H.Remapper(ffi, CM.family(name, *size), size, inp) as r:
            for out in ("bgr", "nv12"):
                H.assert_equal(r.remap(raw, out), SO.bgr_to_nv12(want) if out == "nv12" else want, "%s %s -> %s, plan off" % (name, inp, out))
        print("ok", name, inp, flush=True)
    print("worker OK %d cases" % len(cases), flush=True)


if __name__ == "__main__":
    main()
