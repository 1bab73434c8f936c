"""Caller-made remap tables (tests/_caller_maps.py) through bevw_remapper_from_maps on the GPU: the plan's unit kernel, its per-tap kernel
with slow entries packed as sx | sy << 16, k_plan_build, the NV12 / 4:2:2 / surface translations of scattered group lists, the NV12 store
stage and k_remap_lut -- held to include/bevwarp.h's promise that caller-made maps get cv2.remap's result for every input format, both
output formats and both tie rules.

The expected value is always oracle.remap (which tests/test_caller_maps_host.py holds to the NumPy statement of the formula on the same
maps) of the BGR frames the NumPy specifications (tests/_nv12_spec.py, tests/_yuv422_spec.py) make of the input, passed through
tests/_nv12_out_spec.bgr_to_nv12 for NV12 images.  Every comparison is at tolerance 0 over all pixels, the ones whose footprint lies
outside the frame included.  Which path of the plan a family takes is the host leg's statement.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import _caller_maps as CM
from tests import _nv12_out_spec as SO
from tests import _nv12_spec as S
from tests import _nv12_surfaces as SF
from tests import _yuv422_spec as Y
from tests._harness import Remapper, assert_equal, ffi, run_child  # noqa: F401

pytestmark = pytest.mark.gpu

INPUTS = ("bgr", "nv12", "yuyv", "uyvy")
OUTPUTS = ("bgr", "nv12")
BATCH = 3
PATH_FAMILIES = ("scatter", "extremes", "corner", "transpose")   # the per-tap kernel's cases and one the units take whole
CHILD_TIMEOUT = 180   # seconds: a library load and 16 x 3 small remappers take a few seconds


_frames, _want = {}, {}


def frames_of(sw, sh, inp):
    """BATCH random frames of sw x sh texels as the library takes them in format `inp`, and the BGR frames the specification makes of them
    (made once per size and format; 'yuyv' and 'uyvy' read the same bytes)."""
    key = (sw, sh, "yuv422" if inp in Y.ORDERS else inp)
    if key not in _frames:
        rng = np.random.default_rng([sw, sh, INPUTS.index(inp) if inp not in Y.ORDERS else 2])
        if inp == "bgr":
            _frames[key] = rng.integers(0, 256, (BATCH, sh, sw, 3), dtype=np.uint8)
        elif inp == "nv12":
            _frames[key] = S.random_nv12(rng, (BATCH,), sw, sh)
        else:
            _frames[key] = Y.random_yuv422(rng, (BATCH,), sw, sh)
    raw = _frames[key]
    bkey = (sw, sh, inp, "bgr")
    if bkey not in _frames:
        _frames[bkey] = raw if inp == "bgr" else S.nv12_to_bgr(raw) if inp == "nv12" else Y.yuv422_to_bgr(raw, inp)
    return raw, _frames[bkey]


def want_of(oracle, name, size, inp, out="bgr", variant=0):
    """oracle.remap of the specification's BGR frames through family `name` (computed once per case and left unchanged); NV12 images through
    the output specification.  variant: the oracle.VARIANT_REMAP the value is computed under -- set here and put back afterwards."""
    key = (name, size, inp, variant)
    if key not in _want:
        sw, sh, dw, dh = size
        m1, m2 = CM.family(name, sw, sh, dw, dh)
        before = oracle.get_variant(oracle.VARIANT_REMAP)
        try:
            oracle.set_variant(oracle.VARIANT_REMAP, variant)
            _want[key] = np.stack([oracle.remap(f, m1, m2) for f in frames_of(sw, sh, inp)[1]])
        finally:
            oracle.set_variant(oracle.VARIANT_REMAP, before)
        _want[key].setflags(write=False)
    return SO.bgr_to_nv12(_want[key]) if out == "nv12" else _want[key]


def check_pairs(ffi, oracle, name, size, inputs, outputs):
    for inp in inputs:
        raw = frames_of(size[0], size[1], inp)[0]
        with Remapper(ffi, CM.family(name, *size), size, inp) as r:
            for out in outputs:
                assert_equal(r.remap(raw, out), want_of(oracle, name, size, inp, out), "%s %s -> %s at %s" % (name, inp, out, size))


# ---------------------------------------------------------------------------------------------------------------
# 1. the maps come back as the caller gave them, and BGR frames at batch 3 give cv2.remap's images
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CM.FAMILIES)
def test_maps_round_trip_and_bgr(ffi, oracle, name):
    size = CM.sizes(name)[0]
    with Remapper(ffi, CM.family(name, *size), size, "bgr") as r:
        g1, g2 = np.full_like(r.m1, 0x5a5a), np.full_like(r.m2, 0x5a5a)
        ffi.check(r.L.bevw_remapper_get_maps(r.r, ffi.ptr(g1), ffi.ptr(g2)))
        assert g1.tobytes() == r.m1.tobytes() and g2.tobytes() == r.m2.tobytes()
        dims = (C.c_int32 * 4)()
        ffi.check(r.L.bevw_remapper_dims(r.r, dims))
        assert tuple(dims) == size
        assert_equal(r.remap(frames_of(size[0], size[1], "bgr")[0], "bgr"), want_of(oracle, name, size, "bgr"), name)


# ---------------------------------------------------------------------------------------------------------------
# 2. every input format x every output format; the four large families at 1280 x 960 with BGR and NV12 frames
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CM.FAMILIES)
def test_every_format_pair(ffi, oracle, name):
    for size in CM.sizes(name):
        check_pairs(ffi, oracle, name, size, INPUTS if size != CM.LARGE else ("bgr", "nv12"), OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------
# 3. geometries that select the other paths (csrc/bevw_plan.h: plan_build_impl; csrc/bevwarp.hip: remap_step)
# ---------------------------------------------------------------------------------------------------------------
GEOMETRIES = {
    "src254x192_plan_without_units": ((254, 192, 160, 120), INPUTS, OUTPUTS),     # sw % 4 != 0: the per-tap kernel serves every tile
    "src255x191_no_plan": ((255, 191, 160, 120), ("bgr",), OUTPUTS),              # sw * sh * 3 % 4 != 0: k_remap_lut (odd sizes: BGR frames only)
    "dst158x120_nv12_per_pixel": ((256, 192, 158, 120), INPUTS, OUTPUTS),         # dw % 4 != 0: plan for BGR images, k_remap_lut for NV12 images
    "dst157x119_padded_pitch": ((256, 192, 157, 119), INPUTS, ("bgr",)),          # padded pitch + k_plan_unpad (odd sizes: BGR images only)
}


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("name", PATH_FAMILIES)
def test_geometries_that_select_the_other_paths(ffi, oracle, name, geometry):
    size, inputs, outputs = GEOMETRIES[geometry]
    check_pairs(ffi, oracle, name, size, inputs, outputs)


# ---------------------------------------------------------------------------------------------------------------
# 4. NV12 surfaces at pitch sw + 4, planes shuffled inside one arena: byte for byte the packed result (and the oracle's)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PATH_FAMILIES + ("strip_w",))
def test_nv12_surfaces_equal_packed_frames(ffi, oracle, name):
    size = CM.sizes(name)[0]
    sw, sh = size[:2]
    raw = frames_of(sw, sh, "nv12")[0]
    surf = SF.Surfaces(ffi, raw, sw, sh, sw + 4, layout_seed=71, fill_seed=72, mode="shuffled")
    try:
        with Remapper(ffi, CM.family(name, *size), size, "nv12") as packed, Remapper(ffi, CM.family(name, *size), size, "nv12", pitch=sw + 4) as r:
            for out in OUTPUTS:
                got = r.remap_surfaces(surf.table, out)
                assert_equal(got, want_of(oracle, name, size, "nv12", out), "%s surfaces -> %s" % (name, out))
                assert_equal(got, packed.remap(raw, out), "%s surfaces -> %s against the packed remapper" % (name, out))
    finally:
        surf.free()


# ---------------------------------------------------------------------------------------------------------------
# 5. the other tie rule (BEVW_COMPAT_REMAP 1: half to even, the per-pixel kernel)
# ---------------------------------------------------------------------------------------------------------------
def test_tie_rule_half_to_even(ffi, oracle):
    L = ffi.lib()
    seen_tie = []
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, 1))
        oracle.set_variant(oracle.VARIANT_REMAP, 1)
        for name in CM.FAMILIES:
            size = CM.sizes(name)[0]
            for inp in ("bgr", "nv12"):
                with Remapper(ffi, CM.family(name, *size), size, inp) as r:
                    got = r.remap(frames_of(size[0], size[1], inp)[0], "bgr")
                assert_equal(got, want_of(oracle, name, size, inp, variant=1), "%s %s, ties to even" % (name, inp))
                if not np.array_equal(got, want_of(oracle, name, size, inp)):
                    seen_tie.append(name)
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)
        oracle.set_variant(oracle.VARIANT_REMAP, 0)
    assert seen_tie, "no family hit an exact tie: the rule was not exercised"


# ---------------------------------------------------------------------------------------------------------------
# 6. the plan switched off (BEVW_REMAP_PLAN=0, read once per process): k_remap_lut on the whole catalogue, in a fresh child
# ---------------------------------------------------------------------------------------------------------------
def test_plan_switched_off(oracle, tmp_path):
    z = {}
    for name, size, inp in CM.child_cases():
        z["raw_%d_%d_%s" % (size[0], size[1], inp)] = frames_of(size[0], size[1], inp)[0]
        z["want_%s_%s" % (name, inp)] = want_of(oracle, name, size, inp)
    case_file = str(tmp_path / "case.npz")
    np.savez(case_file, **z)
    run_child("_caller_maps_worker.py", [case_file], {"BEVW_REMAP_PLAN": "0"}, timeout=CHILD_TIMEOUT, expect="worker OK %d cases" % len(CM.child_cases()))
