#!/usr/bin/env python3
"""Golden digests for tests/test_reference_structure.py from the REFERENCE's own Python modules.

Run with a checkout of the reference (dyfcalid/CameraCalibration), after `make -C oracle`:

    BEVW_REFERENCE_ROOT=/path/to/CameraCalibration python tests/golden/make_reference_structure_goldens.py

The reference's SurroundBirdEyeView/surroundBEV.py and ExtrinsicCalibration/extrinsicCalib.py run with `cv2` replaced by the
oracle's primitives (tests/_cv2_shim.py) on the repository's sample rig (tests/golden/repo_rig.npz).  Every array the tests hold
the oracle's restatement against -- rig files, undistort matrices, BEV maps, masks, blend weights, whole BEV images, balance
helpers, the extrinsic pre-processing -- is stored as _golden_cases.value_digest (shape + values), together with the few scalars
the reference derives on the way (board size, scale factors).  Writes tests/golden/reference_structure.json.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _golden_cases as GC  # noqa: E402

REF = os.environ.get("BEVW_REFERENCE_ROOT", "")
OUT = os.path.join(HERE, "reference_structure.json")
CAMS, FLOWS, SQUARES, flow_key = GC.CAMS, GC.REFERENCE_FLOWS, GC.REFERENCE_SQUARES, GC.reference_flow_key


def load_reference_module(relpath, name):
    import _cv2_shim

    _cv2_shim.install()
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def main() -> int:
    if not REF or not os.path.isdir(REF):
        print("set BEVW_REFERENCE_ROOT to a checkout of the reference (found: %r)" % REF, file=sys.stderr)
        return 1
    from conftest import RepoRig

    rig = RepoRig()
    vd = GC.value_digest
    g = {}
    for n in CAMS:
        base = os.path.join(REF, "SurroundBirdEyeView", "data", n)
        for kind in "KDH":
            g["rig/%s/%s" % (n, kind)] = vd(np.load(os.path.join(base, "camera_%s_%s.npy" % (n, kind))))

    sb = load_reference_module("SurroundBirdEyeView/surroundBEV.py", "reference_surroundBEV")
    frames = rig.frames()
    for blend, balance, car_size in FLOWS:
        args = sb.BevGenerator.get_args()
        args.CAR_WIDTH, args.CAR_HEIGHT = car_size            # main.py:79-81 uses 200 x 350, the module default is 250 x 400
        gen = sb.BevGenerator(blend=blend, balance=balance)
        k = flow_key(blend, balance, car_size)
        for i, n in enumerate(CAMS):
            g[k + "/%s/K_dst" % n] = vd(gen.cameras[i].camera_mat_dst)
            g[k + "/%s/bev_map0" % n] = vd(gen.cameras[i].bev_maps[0])
            g[k + "/%s/bev_map1" % n] = vd(gen.cameras[i].bev_maps[1])
            g[k + "/%s/mask" % n] = vd(gen.masks[i].mask)
            if blend:
                g[k + "/%s/weight" % n] = vd(gen.masks[i].weight)
        car = sb.padding(rig.image("car"), args.BEV_WIDTH, args.BEV_HEIGHT)
        g[k + "/car_padded"] = vd(car)
        for tag, c in (("nocar", None), ("car", car)):
            got = gen(*[f.copy() for f in frames], car=c)
            g[k + "/out_%s" % tag] = vd(got)
            g[k + "/out_%s_dtype" % tag] = str(got.dtype)
    for i, out in enumerate(sb.luminance_balance([f.copy() for f in frames])):
        g["balance/luminance/%d" % i] = vd(out)
    g["balance/color_back"] = vd(sb.color_balance(rig.image("back").copy()))
    sys.modules.pop("cv2", None)

    ec = load_reference_module("ExtrinsicCalibration/extrinsicCalib.py", "reference_extrinsicCalib")
    img = rig.image("back")[:301, :403]
    center = ec.CenterImage.__new__(ec.CenterImage)
    center.x, center.y = 100, 250
    g["excalib/translate_100_250"] = vd(center.translate(img))
    a = ec.args
    g["excalib/board"] = [int(a.BORAD_WIDTH), int(a.BORAD_HEIGHT)]
    gx, gy = np.meshgrid(np.arange(a.BORAD_WIDTH), np.arange(a.BORAD_HEIGHT))
    for square in SQUARES:
        corners = np.stack([100 + gx * square, 50 + gy * square], -1).reshape(-1, 2).astype(np.float32)
        sc = ec.ScaleImage(corners)
        g["excalib/scale/%g/factor" % square] = float(sc.scale_factor)
        g["excalib/scale/%g" % square] = vd(sc(img))
    sys.modules.pop("cv2", None)

    with open(OUT, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, len(g), "entries")
    return 0


if __name__ == "__main__":
    sys.exit(main())
