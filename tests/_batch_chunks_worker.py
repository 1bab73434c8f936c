"""Worker of tests/test_batch_chunks_gpu.py: one fresh process per BEVW_PLAN_* switch (the library reads them once per process).

argv: case_dir name value.  The parent sets `name`=`value` in this process's environment and leaves the pool of 143 frame sets, the car
sprite and the expected images (CPU oracle on the _nv12_spec-converted frames) as .npy files in case_dir.  Direct, blend and blend +
balance handles with packed BGR in and BGR out, and one surfaces -> NV12 blend handle, run batches 143, 17 and 63 through the device
entries, each run with the sentinel fill and the guard image of tests/_harness.run_batches, every image compared with tolerance 0.  Any refusal
by the library ends the worker with its error."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _harness as H  # noqa: E402


def main():
    case_dir, name, value = sys.argv[1], sys.argv[2], sys.argv[3]
    ffi, SB = H.worker_library({name: value}, only=("BEVW_PLAN_",))
    z = lambda n: np.load(os.path.join(case_dir, n + ".npy"), mmap_mode="r")
    nb_env = int(value) if name == "BEVW_PLAN_NB" else 0
    inputs = H.Inputs(ffi, np.asarray(z("nv")), np.asarray(z("bgr")), np.asarray(z("car")))
    try:
        for m, (blend, balance) in enumerate(H.WORKER_MODES):
            want = (z("want%d" % m), None, np.asarray(z("none%d" % m)))
            H.stitch_handle(ffi, SB, inputs, want, "bgr", "bgr", blend, balance, batches=H.WORKER_BATCHES, nb_env=nb_env, host_entry=False)
            print("ok bgr -> bgr, blend %d balance %d" % (blend, balance), flush=True)
            if (blend, balance) == (True, False):
                want = (want[0], z("want_nv12_%d" % m), want[2])
                H.stitch_handle(ffi, SB, inputs, want, "surfaces", "nv12", blend, balance, batches=H.WORKER_BATCHES, nb_env=nb_env, host_entry=False)
                print("ok surfaces -> nv12, blend %d balance %d" % (blend, balance), flush=True)
    finally:
        inputs.free()
    print("worker OK %s=%s" % (name, value), flush=True)


if __name__ == "__main__":
    main()
