"""Worker of tests/test_batch_loops_gpu.py: one fresh process per BEVW_PLAN_* switch (the library reads them once per process).

argv: case_dir name value.  The parent sets `name`=`value` in this process's environment and leaves the pools and the expected images of
tests/_batch_loops.py as .npy files in case_dir.  The four one-channel remappers (linear and nearest at 8 and 16 bits), the direct and the
blend one-channel stitch and one YUYV blend handle run batches 143, 17 and 63 through the device entries, each run with the sentinel fill
and the guard image of tests/_harness.run_batches, every image compared with tolerance 0 and every step's path asserted.  Any refusal by the
library ends the worker with its error."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _batch_loops as BL  # noqa: E402
from tests import _harness as H  # noqa: E402


def main():
    case_dir, name, value = sys.argv[1], sys.argv[2], sys.argv[3]
    ffi, SB = H.worker_library({name: value}, only=("BEVW_PLAN_",))
    z = lambda n: np.load(os.path.join(case_dir, n + ".npy"), mmap_mode="r")
    nb_env = int(value) if name == "BEVW_PLAN_NB" else 0
    bufs = []

    def device(a):
        a = np.asarray(a)
        bufs.append(ffi.DeviceBuffer(a.nbytes).upload(a))
        return bufs[-1]

    try:
        dev = {depth: device(z("frames%d" % depth)) for depth in (8, 16)}
        for kind, depth in BL.REMAPPERS:
            want = (z("want_%s%d" % (kind, depth)), np.asarray(z("fixed_%s%d" % (kind, depth))))
            BL.run_remapper(ffi, kind, depth, dev[depth], want, H.WORKER_BATCHES, nb_env=nb_env)
            print("ok remap %s, depth %d" % (kind, depth), flush=True)
        d_gray, car = device(z("gray")), np.asarray(z("gray_car"))
        d_car = device(car)
        for blend in (False, True):
            want = (z("gray_want%d" % blend), np.asarray(z("gray_none%d" % blend)))
            BL.run_gray_stitch(ffi, SB, d_gray, d_car, car, want, blend, H.WORKER_BATCHES, nb_env=nb_env)
            print("ok grey stitch, blend %d" % blend, flush=True)
    finally:
        for d in bufs:
            d.free()
    raw = np.asarray(z("yuyv"))
    inputs = H.Inputs(ffi, raw, None, np.asarray(z("car")), yuv422={"yuyv": raw})
    try:
        want = (z("yuyv_want"), None, np.asarray(z("yuyv_none")))
        bev = H.stitch_handle(ffi, SB, inputs, want, "yuyv", "bgr", True, False, batches=H.WORKER_BATCHES, nb_env=nb_env, host_entry=False)
        assert bev.last_path() == ffi.PATH_UNITS
        print("ok yuyv -> bgr, blend 1", flush=True)
    finally:
        inputs.free()
    print("worker OK %s=%s" % (name, value), flush=True)


if __name__ == "__main__":
    main()
