"""Caller-made remap tables (tests/_caller_maps.py) through the host plan compiler and the emulated unit kernel -- WITHOUT a GPU.

bevw_remapper_from_maps compiles the caller's map1 / map2 into the plan the stitch uses; the unit schedule of that plan was written for the
smooth maps a calibrated fisheye camera gives.  Here every family of the catalogue -- folds, mirrors, transposes, jumps, scatter, a point,
frame edges, the int16 limits, strip-shaped sources -- runs through tests/native/unit_emulate.cpp (unit_compile + the emulated kernel body),
on a plain build and on one under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program; nothing is loaded into Python), and
  * every pixel a unit claims equals the NumPy statement of cv2.remap's fixed-point formula (_caller_maps.numpy_remap),
  * every pixel no unit claims is 0 (the emulator itself checks that every claimed quad is stored exactly once),
  * oracle.remap equals the NumPy statement on the same map (the GPU leg, tests/test_caller_maps_gpu.py, takes it as its expected value),
  * the share of pixels the units take is at least FLOOR[family]: the floors say which path a family exercises -- the unit kernel, or the
    per-tap kernel the units leave the rest to -- so that this leg cannot go green on a compiler that quietly hands everything to the per-tap
    kernel.  They are no correctness bar.  Families without a floor (scatter, extremes, corner, the strips) are the per-tap kernel's cases;
    the share they reach is printed."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import _caller_maps as CM
from tests import _native_build
from tests._native_build import run_units as _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not _native_build.hipcc_path(), reason="hipcc not available")

FLOOR = dict(transpose=0.9, mirror=0.9, quadswap=0.9, constant=0.9, stripes=0.9, rowshuffle=0.9, colshuffle=0.9, minify8=0.9, magnify16=0.9,
             rot180=0.9, rot45=0.9, swirl=0.7, jitter40=0.7)
CASES = [(name, size) for name in CM.FAMILIES for size in CM.sizes(name)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("caller_maps_" + request.param) / "unit_emulate")
    _native_build.build(os.path.join(ROOT, "tests", "native", "unit_emulate.cpp"), out, sanitize=request.param == "sanitized")
    return out


def frames_for(name, size, nframes):
    sw, sh = size[:2]
    rng = np.random.default_rng([CM.FAMILIES.index(name), sw, sh])
    return rng.integers(0, 256, (nframes, 1, sh, sw, 3), dtype=np.uint8)


@pytest.mark.parametrize("name,size", CASES, ids=["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASES])
def test_family_on_the_unit_schedule(exe, tmp_path, name, size):
    sw, sh, dw, dh = size
    m1, m2 = CM.family(name, sw, sh, dw, dh)
    a1, a2 = CM.family(name, sw, sh, dw, dh)
    assert np.array_equal(m1, a1) and np.array_equal(m2, a2)                      # deterministic
    assert m1.shape == (dh, dw, 2) and m1.dtype == np.int16 and m2.shape == (dh, dw) and m2.dtype == np.uint16
    if name != "magnify16":
        assert (m2 >> 10).any()                                                    # bits above bit 9 are set
    frames = frames_for(name, size, 2 if size == CM.SMALL else 1)
    got = _run(exe, tmp_path, [(m1, m2)], [np.full((dh, dw), 255, np.uint8)], frames, None, sw, sh, dw, dh)
    w = got["written"] == 1
    assert set(np.unique(got["written"]).tolist()) <= {0, 1}
    O.build()
    for b in range(frames.shape[0]):
        want = CM.numpy_remap(frames[b, 0], m1, m2)
        assert np.array_equal(O.remap(frames[b, 0], m1, m2), want), "oracle.remap differs from the NumPy statement"
        assert np.array_equal(got["img"][b][w], want[w]), "%s: %d claimed pixels differ" % (name, int((got["img"][b][w] != want[w]).any(-1).sum()))
        assert not got["img"][b][~w].any(), "%s: an unclaimed pixel was written" % name
    share = float(w.mean())
    print("%s %dx%d -> %dx%d: %d units, written share %.3f" % (name, sw, sh, dw, dh, got["units"], share))
    if name in FLOOR:
        assert got["units"] > 0 and share >= FLOOR[name], "%s: the units take %.3f of the image, floor %.1f" % (name, share, FLOOR[name])
    assert (got["units"] > 0) == bool(w.any())


def test_corner_holds_every_value_on_either_side_of_each_edge():
    """`corner` is the family whose every base tile is a border tile: on x every value of -1 .. 3 and sw - 6 .. sw - 1, on y every value of
    -1 .. 2 and sh - 3 .. sh - 1 -- footprints that cross the left, right, top and bottom edge (sx = -1, sx = sw - 1, sy = -1, sy = sh - 1),
    in every geometry the GPU leg runs it at."""
    for sw, sh, dw, dh in (CM.SMALL, (254, 192, 160, 120), (255, 191, 160, 120), (256, 192, 158, 120), (256, 192, 157, 119)):
        m1, _ = CM.family("corner", sw, sh, dw, dh)
        assert set(np.unique(m1[..., 0]).tolist()) == set(range(-1, 4)) | set(range(sw - 6, sw))
        assert set(np.unique(m1[..., 1]).tolist()) == set(range(-1, 3)) | set(range(sh - 3, sh))
        # every base tile of 32 x 8 pixels holds a footprint that crosses the right edge and one that crosses the bottom edge
        for ty in range(0, dh - 7, 8):
            for tx in range(0, dw - 31, 32):
                t = m1[ty:ty + 8, tx:tx + 32]
                assert (t[..., 0] == sw - 1).any() and (t[..., 1] == sh - 1).any() and (t[..., 0] == -1).any() and (t[..., 1] == -1).any()


def test_two_hostile_cameras_blended(exe, tmp_path):
    """`transpose` and `rot180` as the two cameras of a blend: a weight ramp, its complement, and a hole where neither contributes; the
    expected value is min(255, sum over the cameras of (v * (m * 32897)) >> 23) -- the integer form of trunc(f32(v) * f32(m / 255))."""
    sw, sh, dw, dh = CM.SMALL
    luts = [CM.family("transpose", sw, sh, dw, dh), CM.family("rot180", sw, sh, dw, dh)]
    y, x = np.mgrid[0:dh, 0:dw]
    wa = np.clip((x - 40) * 4, 0, 255).astype(np.uint8)
    wb = (255 - wa).astype(np.uint8)
    wa[50:70, 60:100] = 0
    wb[50:70, 60:100] = 0
    frames = np.random.default_rng(77).integers(0, 256, (3, 2, sh, sw, 3), dtype=np.uint8)
    got = _run(exe, tmp_path, luts, [wa, wb], frames, None, sw, sh, dw, dh, True)
    w = got["written"] == 1
    assert got["units"] > 0 and w.mean() >= 0.9, got["log"]
    for b in range(3):
        want = np.zeros((dh, dw, 3), np.int64)
        for c, m in enumerate((wa, wb)):
            v = CM.numpy_remap(frames[b, c], *luts[c]).astype(np.int64)
            want += (v * (m.astype(np.int64) * 32897)[..., None]) >> 23
        want = np.minimum(255, want)
        assert np.array_equal(got["img"][b][w], want[w]) and not got["img"][b][~w].any(), "frame %d" % b
    print("two cameras blended: %d units, written share %.3f" % (got["units"], w.mean()))

