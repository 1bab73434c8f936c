"""Holds the oracle's restatement of the whole path against what the REFERENCE's own Python modules compute: same frames in,
same bytes out.  This pins the structure of the restatement -- operation order, mask polygons, seam lines, blend-weight loop,
padding, luminance / white balance composition, pad / crop rules -- against the reference itself.

The reference side is stored: tests/golden/make_reference_structure_goldens.py runs the reference's surroundBEV.py and
extrinsicCalib.py with `cv2` replaced by the oracle's primitives (tests/_cv2_shim.py) on the sample rig of
tests/golden/repo_rig.npz and writes the value digest of every array compared here to tests/golden/reference_structure.json."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import _golden_cases as GC  # noqa: E402

CAMS, SQUARES, flow_key = GC.CAMS, GC.REFERENCE_SQUARES, GC.reference_flow_key


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "reference_structure.json")) as f:
        return json.load(f)


def same(golden, key, arr):
    assert key in golden, "%s is not in tests/golden/reference_structure.json" % key
    assert GC.value_digest(arr) == golden[key], "%s differs from the reference's (shape %s)" % (key, np.shape(arr))


def test_reference_rig_files_equal_the_fixture(golden, repo_rig):
    for n in CAMS:
        for kind, want in zip("KDH", repo_rig.rig[n]):
            same(golden, "rig/%s/%s" % (n, kind), want)


@pytest.mark.parametrize("blend,balance,car_size", GC.REFERENCE_FLOWS)
def test_reference_control_flow_equals_the_restatement(golden, oracle, repo_rig, blend, balance, car_size):
    k = flow_key(blend, balance, car_size)
    cfg = dict(oracle.DEFAULT_CFG, CAR_WIDTH=car_size[0], CAR_HEIGHT=car_size[1])
    ref = oracle.RefBevGenerator(repo_rig.rig, cfg, blend=blend, balance=balance)
    for i, n in enumerate(CAMS):
        same(golden, k + "/%s/K_dst" % n, ref.cameras[i].K_dst)
        same(golden, k + "/%s/bev_map0" % n, ref.cameras[i].bev_maps[0])
        same(golden, k + "/%s/bev_map1" % n, ref.cameras[i].bev_maps[1])
        same(golden, k + "/%s/mask" % n, ref.masks[i])
        if blend:
            same(golden, k + "/%s/weight" % n, np.repeat(ref.weights[i][:, :, None], 3, axis=2) if ref.weights[i].ndim == 2 else ref.weights[i])
    frames = repo_rig.frames()
    car = oracle.padding(repo_rig.image("car"), cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"])
    same(golden, k + "/car_padded", car)
    for tag, c in (("nocar", None), ("car", car)):
        want = ref(*frames, car=c)
        assert golden[k + "/out_%s_dtype" % tag] == "uint8" and want.dtype == np.uint8
        same(golden, k + "/out_%s" % tag, want)


def test_reference_balance_helpers_equal_the_restatement(golden, oracle, repo_rig):
    frames = repo_rig.frames()
    for i, w in enumerate(oracle.luminance_balance(frames)):
        same(golden, "balance/luminance/%d" % i, w)
    same(golden, "balance/color_back", oracle.color_balance(repo_rig.image("back")))


def test_reference_excalib_preprocessing_equals_the_mirror_rules(golden, oracle, repo_rig):
    img = repo_rig.image("back")[:301, :403]
    h, w = img.shape[:2]
    same(golden, "excalib/translate_100_250", oracle.translate(img, w // 2 - 100, h // 2 - 250))
    assert golden["excalib/board"] == [7, 6]
    for square in SQUARES:
        factor = golden["excalib/scale/%g/factor" % square]
        assert factor == 10.0 / square   # ScaleImage: args.SCALED_SIZE / the mean corner distance of the synthetic board (extrinsicCalib.py:91)
        ref = oracle.resize_linear(img, factor, factor)
        if factor < 1:
            want = np.zeros_like(img)
            t, l = (h - ref.shape[0]) // 2, (w - ref.shape[1]) // 2
            want[t:t + ref.shape[0], l:l + ref.shape[1]] = ref
        else:
            t, l = (ref.shape[0] - h) // 2, (ref.shape[1] - w) // 2
            want = ref[t:t + h, l:l + w]
        same(golden, "excalib/scale/%g" % square, want)
