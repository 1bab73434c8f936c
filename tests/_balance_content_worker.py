"""Worker of tests/test_balance_content_gpu.py: one fresh process per set of balance switches (BEVW_BAL_PARTS, BEVW_BAL_RING, BEVW_BAL_MODE,
BEVW_GAIN_OOP: the library reads each once per process).

argv: case_dir NAME=VALUE [NAME=VALUE ...].  The parent sets the switches in this process's environment and leaves the pool of
tests/_balance_content.py (BGR and NV12 forms), the car sprite and the expected images (CPU oracle on the frames, on the
_nv12_spec-converted frames for NV12) as .npy files in case_dir.  A blend + balance handle per pixel format -- BGR in and out, NV12 in and
out -- runs batch 33 twice in a row through the device entry, so that ring slots and scratch buffers are reused, each run with the sentinel
fill and the guard image of tests/_harness.run_batches, every image compared with tolerance 0.  Any refusal by the library ends the
worker with its error."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _harness as H  # noqa: E402

PREFIXES = ("BEVW_BAL_", "BEVW_GAIN_", "BEVW_PLAN_")


def main():
    case_dir, switches = sys.argv[1], dict(a.split("=", 1) for a in sys.argv[2:])
    name = " ".join(sys.argv[2:])
    assert switches, name
    ffi, SB = H.worker_library(switches, only=PREFIXES)
    z = lambda n: np.load(os.path.join(case_dir, n + ".npy"), mmap_mode="r")
    inputs = H.Inputs(ffi, np.asarray(z("nv")), np.asarray(z("bgr")), np.asarray(z("car")))
    try:
        for fmt in ("bgr", "nv12"):
            want = (z("want_" + fmt), z("want_nv12_out") if fmt == "nv12" else None, np.asarray(z("none")))
            H.stitch_handle(ffi, SB, inputs, want, fmt, fmt, True, True, batches=(33, 33), host_entry=False, one_slice=True)
            print("ok %s -> %s, blend 1 balance 1, batch 33 twice" % (fmt, fmt), flush=True)
    finally:
        inputs.free()
    print("worker OK %s" % name, flush=True)


if __name__ == "__main__":
    main()
