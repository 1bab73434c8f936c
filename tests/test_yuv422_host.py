"""Packed 4:2:2 camera frames (input_format='yuyv' / 'uyvy') checked WITHOUT a GPU.

  * tests/native/yuv422_emulate.cpp compiles, for the host, the translation of a unit's group list into 4:2:2 offsets (bevw_unit.h:
    unit_gsrc_yuv422) and the landing of one 16-byte texel group into the four pair entries of the unit kernel's LDS patch (bevw_pair.h:
    pair_convert_yuv422 with the byte order's v_perm selectors).  Both byte orders are compared here with pair entries built from the
    NumPy specification's BGR texels (tests/_yuv422_spec.py), the offsets with the bytes they must address;
  * the built library: the kernels that read 4:2:2 frames live in a translation unit of their own (build.FORMAT_UNITS), which shares no
    kernel with build.UNITS, and the unit kernels' metadata stays inside the family's resource budget;
  * the public surface: header constants, ABI version, the Python argument checks that need no device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import _yuv422_spec as S

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
NO_GROUP = 0x80000000   # kPairNoGroup (bevw_pair.h)
ORDER_VALUE = {"yuyv": 4, "uyvy": 5}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests import _native_build

    path = str(tmp_path_factory.mktemp("yuv422") / "yuv422_emulate")
    _native_build.build(os.path.join(ROOT, "tests", "native", "yuv422_emulate.cpp"), path)
    return path


def _land(exe, tmp_path, order, fw, fh, ncams, frame_set, gsrc):
    paths = [str(tmp_path / n) for n in ("set.bin", "gsrc.bin", "offs.bin", "pairs.bin")]
    frame_set.tofile(paths[0])
    np.asarray(gsrc, np.uint32).tofile(paths[1])
    r = subprocess.run([exe, "land", str(ORDER_VALUE[order]), str(fw), str(fh), str(ncams)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(paths[2], np.uint32), np.fromfile(paths[3], np.uint8).reshape(-1, 4, 8)


@needs_hipcc
@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("fw,fh,ncams", [(16, 6, 4), (24, 10, 1), (8, 3, 4)])   # (8, 3): an odd height, which NV12 cannot have
def test_group_offsets_and_landing(exe, tmp_path, fw, fh, ncams, order):
    """Every group of a synthetic frame set, in shuffled order -- the last of each row and the last of the whole set among them -- and slots
    without a group: the offset addresses the group's bytes, and the landed pair entries are pair_convert's entries of the specification's
    BGR texels (zeros for a slot without a group)."""
    rng = np.random.default_rng(fw * 1000 + fh * 10 + ncams + ORDER_VALUE[order])
    gpr = fw // 4
    frames = S.random_yuv422(rng, (ncams,), fw, fh)
    ngroups = ncams * fh * gpr
    gsrc = [12 * k for k in range(ngroups)] + [NO_GROUP] * 3
    gsrc = [gsrc[i] for i in rng.permutation(len(gsrc))]
    offs, pairs = _land(exe, tmp_path, order, fw, fh, ncams, frames.reshape(-1), gsrc)
    flat = frames.reshape(-1)
    bgr = S.yuv422_to_bgr(frames, order)   # [ncams, fh, fw, 3]
    seen_row_end = seen_set_end = 0
    for slot, g in enumerate(gsrc):
        if g == NO_GROUP:
            assert int(offs[slot]) == NO_GROUP
            assert not pairs[slot].any(), "a slot without a group must land zero pair entries"
            continue
        k = g // 12
        cam, rem = divmod(k, fh * gpr)
        y, x = rem // gpr, 4 * (rem % gpr)
        o = int(offs[slot])
        assert o == 2 * (cam * fw * fh + y * fw + x) and o % 8 == 0
        assert np.array_equal(flat[o:o + 8], frames[cam, y, x:x + 4].reshape(-1))
        for p in range(4):
            a, b = x + p, x + p + 1
            want = np.zeros(8, np.uint8)
            want[[0, 2, 4]] = bgr[cam, y, a]
            if b < fw:
                want[[1, 3, 5]] = bgr[cam, y, b]
                assert np.array_equal(pairs[slot, p], want), (slot, cam, y, x, p)
            else:   # texel x+4 of a row's last group lies outside the frame: no unit pixel samples it, its bytes are unspecified
                assert np.array_equal(pairs[slot, p, [0, 2, 4, 6, 7]], want[[0, 2, 4, 6, 7]]), (slot, cam, y, x, p)
        seen_row_end += x + 4 == fw
        seen_set_end += k == ngroups - 1
    assert seen_row_end == ncams * fh and seen_set_end == 1


def test_spec_layouts_and_round_trip():
    """The two byte orders read the same components from their own positions, and the input generator keeps grey (nearly) grey."""
    rng = np.random.default_rng(2)
    f = S.random_yuv422(rng, (2,), 8, 3)
    swapped = f[..., ::-1]   # the same components in the other order
    assert np.array_equal(S.yuv422_to_bgr(f, "yuyv"), S.yuv422_to_bgr(swapped, "uyvy"))
    one = np.array([[[50, 90], [60, 200]]], np.uint8)   # YUYV: Y0 50 U 90 Y1 60 V 200
    from tests import _nv12_spec as N

    assert np.array_equal(S.yuv422_to_bgr(one, "yuyv")[0], N.yuv_to_bgr(np.array([50, 60]), 90, 200))
    assert np.array_equal(S.yuv422_to_bgr(one, "uyvy")[0], N.yuv_to_bgr(np.array([90, 200]), 50, 60))
    assert S.yuv422_to_bgr(np.zeros((1, 2, 2), np.uint8), "yuyv")[0, 0].tolist() == [0, 154, 0]   # what a lane without a group must NOT land
    img = np.full((3, 6, 3), 128, np.uint8)
    for order in S.ORDERS:
        back = S.yuv422_to_bgr(S.bgr_to_yuv422(img, order), order)
        assert back.shape == img.shape and int(np.abs(back.astype(int) - 128).max()) <= 1


# ---------------------------------------------------------------------------------------------------------------
# the built library
# ---------------------------------------------------------------------------------------------------------------
# the instantiations the host dispatch of bevwarp_yuv422.hip uses: k_units_yuv422<BLEND> 2, k_units_out_yuv422<BLEND> 2,
# k_stitch_plan_yuv422 8 (BLEND x LUM x SUMS, BGR images) + 2 (BLEND, NV12 images), k_stitch_pp_yuv422 4 (BLEND x BAL) + 2 (BLEND, NV12
# images), k_remap_lut_yuv422 2 (BGR / NV12 images), k_vsum_yuv422 1, k_lum_groups_yuv422 1
YUV422_KERNELS = 24
YUV422_FAMILIES = {"k_units_yuv422": 2, "k_units_out_yuv422": 2, "k_stitch_plan_yuv422": 10, "k_stitch_pp_yuv422": 6, "k_remap_lut_yuv422": 2,
                   "k_vsum_yuv422": 1, "k_lum_groups_yuv422": 1}


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    from cameracalibration_amd import build
    from tests import _native_build as TU

    build.build()
    tmp = str(tmp_path_factory.mktemp("yuv422_units"))
    assert build.FORMAT_UNITS == ["bevwarp_yuv422.hip"] and not set(build.FORMAT_UNITS) & set(build.UNITS)
    kernels = {u: TU.kernels_of(os.path.join(build.OBJ, u.replace(".hip", ".o")), tmp) for u in build.UNITS + build.FORMAT_UNITS}
    return kernels, tmp, TU


@needs_hipcc
def test_the_format_unit_holds_its_own_kernels_and_no_others(units):
    from cameracalibration_amd import build

    kernels, _, _ = units
    mine = kernels["bevwarp_yuv422.hip"]
    for u in build.UNITS:
        assert not mine & kernels[u], (u, sorted(mine & kernels[u]))
        assert not {k for k in kernels[u] if "yuv422" in k}, u   # ... and no 4:2:2 kernel lives anywhere else
    assert len(mine) == YUV422_KERNELS, sorted(mine)
    assert all("yuv422" in k for k in mine), sorted(mine)
    assert {f: sum(("k_units_out_yuv422" not in k if f == "k_units_yuv422" else True) and f in k for k in mine) for f in YUV422_FAMILIES} == YUV422_FAMILIES


@needs_hipcc
def test_unit_kernels_stay_inside_the_resource_budget(units):
    """Metadata of the code object only: at most 168 VGPRs (3 waves per SIMD), no private segment, the 32 KB patch in LDS."""
    _, tmp, TU = units
    notes = subprocess.run([os.path.join(TU.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, "bevwarp_yuv422.o.co")], check=True,
                           capture_output=True, text=True, timeout=120).stdout
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "k_units_" not in name.group(1):
            continue
        found[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                                for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len(found) == 4, sorted(found)
    for name, m in found.items():
        print(name, m)
        assert m["vgpr_count"] <= 168 and m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 32768, (name, m)


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------
def test_constants_and_abi():
    from cameracalibration_amd import _ffi, build

    text = open(os.path.join(ROOT, "include", "bevwarp.h")).read()
    consts = {n: int(v) for n, v in re.findall(r"#define BEVW_INPUT_(\w+) (\d+)", text)}
    assert consts == {"BGR": _ffi.INPUT_BGR, "NV12": _ffi.INPUT_NV12, "YUYV": _ffi.INPUT_YUYV, "UYVY": _ffi.INPUT_UYVY}
    assert (_ffi.INPUT_YUYV, _ffi.INPUT_UYVY) == (4, 5)
    assert _ffi.INPUT_FORMATS == {"bgr": 0, "nv12": 1, "yuyv": 4, "uyvy": 5}
    assert "#define BEVW_ABI_VERSION 8" in text and _ffi.ABI_VERSION == 8
    assert "COLOR_YUV2BGR_YUY2" in text and "COLOR_YUV2BGR_UYVY" in text
    for line in text.splitlines():
        if "Not provided" in line:
            assert "YUYV" not in line, line
    build.build()
    L = _ffi.lib()
    assert L.bevw_abi_version() == 8
    # null handles are refused before anything touches a device
    assert L.bevw_set_input_format(None, _ffi.INPUT_YUYV) == -1 and L.bevw_remapper_set_input_format(None, _ffi.INPUT_UYVY) == -1


def test_python_argument_checks_without_a_device():
    from cameracalibration_amd import _ffi
    from cameracalibration_amd import workloads as W
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB
    from cameracalibration_amd.Tools import undistort as U

    assert _ffi.input_format("yuyv") == 4 and _ffi.input_format("uyvy") == 5 and _ffi.input_format("nv12") == 1
    for bad in ("yvyu", "i420", "YUYV", None):
        with pytest.raises(Exception, match="bgr/nv12/yuyv/uyvy"):
            _ffi.input_format(bad)
    assert _ffi.frame_shape("yuyv", 256, 320) == (256, 320, 2) == _ffi.frame_shape("uyvy", 256, 320)
    assert _ffi.frame_shape("nv12", 256, 320) == (384, 320) and _ffi.frame_shape("bgr", 256, 320) == (256, 320, 3)
    # the keywords are checked before any device call
    with pytest.raises(Exception, match="bgr/nv12/yuyv/uyvy"):
        SB.BevGenerator(rig=W.repo_rig(), input_format="yvyu")
    with pytest.raises(Exception, match="input_format='nv12'"):
        SB.BevGenerator(rig=W.repo_rig(), input_format="yuyv", input_pitch=4096)
    K, D = W.undistort_calibration()
    with pytest.raises(Exception, match="bgr/nv12/yuyv/uyvy"):
        U.Undistorter(K, D, 64, 48, input_format="yvyu")
    with pytest.raises(Exception, match="input_format='nv12'"):
        U.Undistorter(K, D, 64, 48, input_format="uyvy", input_pitch=128)
