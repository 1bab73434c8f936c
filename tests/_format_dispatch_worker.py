"""Worker of tests/test_format_dispatch_gpu.py: one fresh process per BEVW_* switch (the library reads them once per process).

argv: case_file switch.  The parent sets `switch`=0 in this process's environment and leaves the inputs and the expected images (CPU
oracle on the _nv12_spec-converted frames) in case_file.  Every input kind (packed BGR, packed NV12, NV12 surfaces at pitch FW + 4) x
output format (BGR, NV12) x (blend, balance) runs with the car sprite and is compared with tolerance 0, uncovered pixels included; under
BEVW_REMAP_PLAN=0 the fisheye undistorter runs over the same inputs and outputs.  Any refusal by the library ends the worker with its
error: none of these combinations is refused."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _harness as H  # noqa: E402
from tests import _nv12_surfaces as SF  # noqa: E402

MODES = ((0, 0), (1, 0), (0, 1), (1, 1))   # (blend, balance)
INPUTS = ("bgr", "nv12", "surfaces")
OUTPUTS = ("bgr", "nv12")


def stitch(ffi, SB, z):
    cfg = H.SMALL_CFG
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    nv, bgr, car = z["nv"], z["bgr"], z["car"]
    surf = SF.Surfaces(ffi, nv.reshape(12, fh * 3 // 2, fw), fw, fh, fw + 4, layout_seed=31, fill_seed=32, mode="shuffled")
    try:
        for m, (blend, balance) in enumerate(MODES):
            want, none = z["want%d" % m], z["none%d" % m]
            for inp in INPUTS:
                for out in OUTPUTS:
                    what = "%s -> %s, blend %d balance %d" % (inp, out, blend, balance)
                    kw = dict(blend=bool(blend), balance=bool(balance), input_format="bgr" if inp == "bgr" else "nv12", output_format=out)
                    if inp == "surfaces":
                        bev = H.generator(SB, H.small_rig(), cfg, input_pitch=fw + 4, **kw)
                        assert bev.plan_info()["schedule"] == ffi.SCHED_TILE_PLAN, what
                        d_out = H.run_table(ffi, bev, surf.table.reshape(3, 4, 2), car, cfg)
                        try:
                            got = [H.fetch(ffi, bev, d_out, cfg, b) for b in range(3)]
                        finally:
                            d_out.free()
                    else:
                        bev = H.generator(SB, H.small_rig(), cfg, **kw)
                        assert bev.plan_info()["schedule"] == ffi.SCHED_TILE_PLAN, what
                        got = bev.batch(bgr if inp == "bgr" else nv, car)
                    for b in range(3):
                        H.check_image(got[b], want[b], none, "%s, set %d" % (what, b), out, black=False)
                    print("ok", what, flush=True)
    finally:
        surf.free()


def undistort(ffi, z):
    from cameracalibration_amd.Tools import undistort as U

    cfg = H.SMALL_CFG
    w, h = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    K, D, _ = H.small_rig()["front"]
    nv, bgr, want, outside = z["nv"][:, 0], z["bgr"][:, 0], z["und_want"], z["und_outside"]
    surf = SF.Surfaces(ffi, nv, w, h, w + 4, layout_seed=33, fill_seed=34, mode="split")
    try:
        for inp in INPUTS:
            for out in OUTPUTS:
                what = "undistort %s -> %s" % (inp, out)
                und = U.Undistorter(K, D, w, h, input_format="bgr" if inp == "bgr" else "nv12", output_format=out,
                                    input_pitch=w + 4 if inp == "surfaces" else None)
                assert (und.out_w, und.out_h) == tuple(z["und_size"]), what
                shape = (3, und.out_h * 3 // 2, und.out_w) if out == "nv12" else (3, und.out_h, und.out_w, 3)
                if inp == "surfaces":
                    d_out = ffi.DeviceBuffer(3 * und.out_image_bytes)
                    d_out.fill(0x5a)
                    try:
                        und.run_surfaces(surf.table, d_out.ptr, out_bytes=d_out.nbytes)
                        und.sync()
                        got = d_out.download(shape)
                    finally:
                        d_out.free()
                else:
                    got = und(bgr if inp == "bgr" else nv)
                    assert got.shape == shape, what
                for b in range(3):
                    H.check_image(got[b], want[b], outside, "%s, image %d" % (what, b), out, black=True)
                und.close()
                print("ok", what, flush=True)
    finally:
        surf.free()


def main():
    case_file, switch = sys.argv[1], sys.argv[2]
    ffi, SB = H.worker_library({switch: "0"})
    z = np.load(case_file)
    stitch(ffi, SB, z)
    if switch == "BEVW_REMAP_PLAN":
        undistort(ffi, z)
    print("worker OK", switch, flush=True)


if __name__ == "__main__":
    main()
