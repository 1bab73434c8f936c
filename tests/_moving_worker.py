"""Worker of tests/test_moving_gpu.py::test_against_a_fresh_generator_under_a_compat_switch: one fresh process per switch, because
bevw_set_compat changes the process-wide defaults that every handle built afterwards snapshots.

argv: key ('warp' | 'remap'), value.  Sets BEVW_COMPAT_WARP / BEVW_COMPAT_REMAP to `value`, then holds the moving step of one handle (the
mixed table, five frame sets, direct and blend) against yardstick B: per frame set a fresh BevGenerator of the rig with H_b on the library's
static path, built under the same switch.  A run under the default switch first says that the switch changes bytes at all."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import _harness as H  # noqa: E402
from tests import _moving as MV  # noqa: E402


def main():
    key, value = sys.argv[1], int(sys.argv[2])
    ffi, SB = H.worker_library({})
    O.build()
    L = ffi.lib()
    compat = {"warp": ffi.COMPAT_WARP, "remap": ffi.COMPAT_REMAP}[key]
    kw = dict(schedule=ffi.SCHED_AUTO, output_pitch="dense")   # (ties to even run the per-pixel schedule: no tile plan, no output pitch)
    rng = np.random.default_rng(1806)
    rig = H.small_rig()
    rigs = MV.mixed_rigs(O, rig)
    frames, car = MV.frames_for(rng, len(rigs)), H.random_car(rng, MV.CFG)
    hs = MV.table(rigs)
    none = H.uncovered(O.RefBevGenerator(rig, MV.CFG))
    for blend in (False, True):
        assert L.bevw_get_compat(compat) == 0
        plain, _ = MV.run_step(ffi, H.generator(SB, rig, MV.CFG, blend=blend, **kw), frames, hs, car)
        ffi.check(L.bevw_set_compat(compat, value))
        try:
            want = MV.library_images(SB, rigs, frames, car, blend, **kw)
            bev = H.generator(SB, rig, MV.CFG, blend=blend, **kw)
            got, path = MV.run_step(ffi, bev, frames, hs, car)
        finally:
            ffi.check(L.bevw_set_compat(compat, 0))
        assert path == ffi.PATH_PER_PIXEL
        MV.assert_images(got, want, none, "yardstick B under %s %d, blend %d" % (key, value, blend))
        changed = int((got != plain).sum())
        assert changed > 0, "the switch changes no byte of these images"
        print("ok blend %d: %d bytes differ from the default switch" % (blend, changed), flush=True)
    print("worker OK %s %d" % (key, value), flush=True)


if __name__ == "__main__":
    main()
