"""The one-channel mode of the remapper (bevw_remapper_set_channels: cv2.remap on a uint8 [H, W] array) -- WITHOUT a GPU.

  * the public surface: the three entry points and BEVW_PATH_* in include/bevwarp.h, ABI 8, null remappers refused before a device is
    touched, the Python keyword checked before any device call;
  * the list translation and the landing: tests/native/gray_emulate.cpp compiles the units of every family of tests/_caller_maps.py as the
    library does, translates their group lists with unit_gsrc_gray, lands every slot as one 8-byte load (dwords past the frames read as
    zero; it fails on a load that straddles the end or is not 4-byte aligned) and runs the unit kernel's lane code through to output
    bytes.  What the units own equals oracle.remap on the 2-D array and, as a second statement, channel 0 of the NumPy formula on the
    replicated image.  The program runs as a plain build and as a stand-alone AddressSanitizer + UndefinedBehaviorSanitizer build;
  * the build: bevwarp_gray.hip's gfx950 code object shares no kernel with another unit, every kernel of it is named *gray*, the three main
    units keep their counts, and k_units_gray stays inside the unit family's budget (metadata notes of the code object only)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import _caller_maps as CM
from tests import _gray_maps as GM
from tests import _native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(not _native_build.hipcc_path(), reason="hipcc not available")

GRAY_FAMILIES = {"k_units_gray": 1, "k_stitch_plan_gray": 1, "k_remap_lut_gray": 1}


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------
def test_header_ffi_and_null_remappers():
    from cameracalibration_amd import _ffi, build

    text = open(os.path.join(ROOT, "include", "bevwarp.h")).read()
    for decl in ("int bevw_remapper_set_channels(bevw_remapper *r, int channels);", "int bevw_remapper_channels(bevw_remapper *r);",
                 "int bevw_remapper_last_path(bevw_remapper *r);"):
        assert decl in text, decl
    paths = {n: int(v) for n, v in re.findall(r"#define BEVW_PATH_(\w+) (\d+)", text)}
    assert paths == {"NONE": _ffi.PATH_NONE, "UNITS": _ffi.PATH_UNITS, "PER_PIXEL": _ffi.PATH_PER_PIXEL} == {"NONE": 0, "UNITS": 1, "PER_PIXEL": 2}
    assert "#define BEVW_ABI_VERSION 8" in text and _ffi.ABI_VERSION == 8
    for name in ("bevw_remapper_set_channels", "bevw_remapper_channels", "bevw_remapper_last_path"):
        assert name in _ffi.SIGNATURES
    # the format axis is untouched
    assert {n: int(v) for n, v in re.findall(r"#define BEVW_INPUT_(\w+) (\d+)", text)} == {"BGR": 0, "NV12": 1, "YUYV": 4, "UYVY": 5}
    assert _ffi.INPUT_FORMATS == {"bgr": 0, "nv12": 1, "yuyv": 4, "uyvy": 5}
    assert build.UNITS == ["bevwarp.hip", "bevwarp_plan.hip", "bevwarp_jpeg.hip"] and build.FORMAT_UNITS == ["bevwarp_yuv422.hip"]
    assert build.CHANNEL_UNITS == ["bevwarp_gray.hip"]
    build.build()
    L = _ffi.lib()
    assert L.bevw_abi_version() == 8
    # null remappers are refused before anything touches a device
    assert L.bevw_remapper_set_channels(None, 1) == -1 and L.bevw_remapper_channels(None) == -1 and L.bevw_remapper_last_path(None) == -1
    assert b"null remapper" in L.bevw_last_error()


def test_python_keyword_checks_without_a_device():
    from cameracalibration_amd import _ffi
    from cameracalibration_amd import workloads as W
    from cameracalibration_amd.Tools import undistort as U

    assert _ffi.channels(1) == 1 and _ffi.channels(3) == 3
    for bad in (0, 2, 4, -1, None, "1", True, 1.5):
        with pytest.raises(Exception, match="channels should be 1/3"):
            _ffi.channels(bad)
    K, D = W.undistort_calibration()
    for bad in (0, 2, 4, None):
        with pytest.raises(Exception, match="channels should be 1/3"):
            U.Undistorter(K, D, 64, 48, channels=bad)
    # one channel is BGR in and out without a pitch: refused before any device call
    for kw in (dict(input_format="nv12"), dict(input_format="yuyv"), dict(output_format="nv12"), dict(input_pitch=64),
               dict(input_format="nv12", input_pitch=128)):
        with pytest.raises(Exception, match="channels=1"):
            U.Undistorter(K, D, 64, 48, channels=1, **kw)
    # ... and the format keywords keep their own messages
    with pytest.raises(Exception, match="bgr/nv12/yuyv/uyvy"):
        U.Undistorter(K, D, 64, 48, channels=1, input_format="i420")
    with pytest.raises(Exception, match="bgr/nv12"):
        U.Undistorter(K, D, 64, 48, channels=1, output_format="i420")


# ---------------------------------------------------------------------------------------------------------------
# list translation, landing, lane code
# ---------------------------------------------------------------------------------------------------------------
CASES = [(name, size) for name in CM.FAMILIES for size in CM.sizes(name)]


def gray_frames(name, size, nframes):
    """Random grey frames that hit every byte value."""
    sw, sh = size[:2]
    rng = np.random.default_rng([7, CM.FAMILIES.index(name), sw, sh])
    f = rng.integers(0, 256, (nframes, sh, sw), dtype=np.uint8)
    assert len(np.unique(f)) == 256
    return f


def _emulate(exe, tmp_path, m1, m2, frames, sw, sh, dw, dh):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i", sw, sh, dw, dh, frames.shape[0]))
        f.write(np.ascontiguousarray(m1, np.int16).tobytes())
        f.write(np.ascontiguousarray(m2, np.uint16).tobytes())
        f.write(np.ascontiguousarray(frames, np.uint8).tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    nunits, = struct.unpack("<i", raw[:4])
    written = np.frombuffer(raw, np.uint8, dw * dh, 4).reshape(dh, dw)
    img = np.frombuffer(raw, np.uint8, frames.shape[0] * dh * dw, 4 + dw * dh).reshape(frames.shape[0], dh, dw)
    return nunits, written, img, r.stdout


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gray_" + request.param) / "gray_emulate")
    _native_build.build(os.path.join(ROOT, "tests", "native", "gray_emulate.cpp"), out, sanitize=request.param == "sanitized")
    return out


@needs_hipcc
@pytest.mark.parametrize("name,size", CASES, ids=["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASES])
def test_family_on_the_gray_units(exe, tmp_path, name, size):
    sw, sh, dw, dh = size
    m1, m2 = CM.family(name, sw, sh, dw, dh)
    frames = gray_frames(name, size, 2 if size == CM.SMALL else 1)
    nunits, written, img, log = _emulate(exe, tmp_path, m1, m2, frames, sw, sh, dw, dh)
    assert set(np.unique(written).tolist()) <= {0, 1}, "a byte was stored twice"
    w = written == 1
    O.build()
    for b in range(frames.shape[0]):
        want = O.remap(frames[b], m1, m2)
        assert want.shape == (dh, dw) and want.dtype == np.uint8
        second = CM.numpy_remap(np.repeat(frames[b][..., None], 3, -1), m1, m2)[..., 0]
        assert np.array_equal(want, second), "oracle.remap on the 2-D array differs from the NumPy statement"
        assert np.array_equal(img[b][w], want[w]), "%s: %d owned pixels differ" % (name, int((img[b][w] != want[w]).sum()))
        assert not img[b][~w].any(), "%s: a pixel no unit owns was written" % name
    print("%s %dx%d -> %dx%d: %d units, owned share %.3f; %s" % (name, sw, sh, dw, dh, nunits, float(w.mean()), log.strip()))
    assert (nunits > 0) == bool(w.any())


@needs_hipcc
def test_the_smooth_families_are_the_units_cases(tmp_path_factory):
    """This leg must not go green on a compiler that hands everything to the per-tap kernel: the smooth families are owned by the units."""
    out = str(tmp_path_factory.mktemp("gray_share") / "gray_emulate")
    _native_build.build(os.path.join(ROOT, "tests", "native", "gray_emulate.cpp"), out)
    sw, sh, dw, dh = CM.SMALL
    for name in ("transpose", "rot180", "magnify16"):
        m1, m2 = CM.family(name, sw, sh, dw, dh)
        nunits, written, _, _ = _emulate(out, tmp_path_factory.mktemp("gray_" + name), m1, m2, gray_frames(name, CM.SMALL, 1), sw, sh, dw, dh)
        assert nunits > 0 and (written == 1).mean() >= 0.9, name


@needs_hipcc
def test_the_frames_last_group_is_never_a_units_group(exe, tmp_path):
    """A smooth shift that ends in the frame's last texel (tests/_gray_maps.py).  The plan is the three-channel one, and its compiler hands
    no group to a unit whose 16-byte BGR window would overrun the frame set (bevw_unit.h, unit_compile: "the last group's window would
    overrun") -- which is exactly the last group of the set's last row, the only group whose 8-byte one-channel load reaches a dword past
    the frames.  So the units own everything but the one 32 x 8 base tile that samples that group (it is the per-tap kernel's, which reads
    single bytes), no unit load reaches past the frames (the emulator counts 0 such dwords and never comes near its "straddles the end"
    failure), and the kernel's range-checked descriptor is a second line of defence that this plan never leans on."""
    sw, sh, dw, dh = CM.SMALL
    m1, m2 = GM.edge_shift(sw, sh, dw, dh)
    assert (m1[-1, -1] == (sw - 2, sh - 2)).all()
    frames = np.random.default_rng(41).integers(0, 256, (2, sh, sw), dtype=np.uint8)
    nunits, written, img, log = _emulate(exe, tmp_path, m1, m2, frames, sw, sh, dw, dh)
    own = written == 1
    # the pixels whose footprint touches the last group of the last row: sx + 1 >= sw - 4 and sy + 1 == sh - 1
    last_group = (m1[..., 0] + 1 >= sw - 4) & (m1[..., 1] + 1 == sh - 1)
    assert last_group.any() and not own[last_group].any()
    left = np.zeros_like(own)
    left[dh - 8:, dw - 32:] = True                                   # the base tile that holds them
    assert np.array_equal(own, ~left), "the units own everything but that base tile"
    assert nunits > 0 and " 0 dwords past the frames read as zero" in log, log
    O.build()
    for b in range(2):
        want = O.remap(frames[b], m1, m2)
        assert np.array_equal(img[b][own], want[own]) and not img[b][~own].any()


@needs_hipcc
def test_the_route_of_a_one_channel_step(tmp_path):
    """tests/native/plan_route_gray.cpp: plan_route with the one-channel format and list, over every input; the other formats' routes do
    not depend on the new list."""
    out = str(tmp_path / "plan_route_gray")
    _native_build.build(os.path.join(ROOT, "tests", "native", "plan_route_gray.cpp"), out)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gray route ok: %d cases" % (2 ** 8 * 2 ** 6) in r.stdout and "other formats ok: %d cases" % (4 * 2 ** 8 * 2 ** 5) in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------
# the built library
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def units(tmp_path_factory):
    from cameracalibration_amd import build
    from tests import _native_build as TU

    build.build()
    tmp = str(tmp_path_factory.mktemp("gray_units"))
    every = build.UNITS + build.FORMAT_UNITS + build.CHANNEL_UNITS
    return {u: TU.kernels_of(os.path.join(build.OBJ, u.replace(".hip", ".o")), tmp) for u in every}, tmp, TU


@needs_hipcc
def test_the_channel_unit_holds_its_own_kernels_and_no_others(units):
    from cameracalibration_amd import build

    kernels, _, _ = units
    mine = kernels["bevwarp_gray.hip"]
    for u in build.UNITS + build.FORMAT_UNITS:
        assert not mine & kernels[u], (u, sorted(mine & kernels[u]))
        assert not {k for k in kernels[u] if "gray" in k}, u   # ... and no one-channel kernel lives anywhere else
    assert mine and all("gray" in k for k in mine), sorted(mine)
    assert {f: sum(f in k for k in mine) for f in GRAY_FAMILIES} == GRAY_FAMILIES and len(mine) == sum(GRAY_FAMILIES.values()), sorted(mine)
    assert {u: len(kernels[u]) for u in build.UNITS} == {"bevwarp.hip": 69, "bevwarp_plan.hip": 54, "bevwarp_jpeg.hip": 24}
    assert len(kernels["bevwarp_yuv422.hip"]) == 24


@needs_hipcc
def test_the_gray_unit_kernel_stays_inside_the_resource_budget(units):
    """Metadata of the code object only: no private segment, LDS <= 32768, at most 168 VGPRs (three waves per SIMD, the family's budget)."""
    _, tmp, TU = units
    notes = subprocess.run([os.path.join(TU.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, "bevwarp_gray.o.co")], check=True,
                           capture_output=True, text=True, timeout=120).stdout
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "k_units_gray" not in name.group(1):
            continue
        found[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                                for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len(found) == 1, sorted(found)
    for name, m in found.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] <= 32768 and m["vgpr_count"] <= 168, (name, m)
