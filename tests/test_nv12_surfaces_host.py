"""NV12 surfaces (bevw_set_input_pitch, bevw_run_surfaces_device) checked WITHOUT a GPU.

  * tests/native/nv12_surf_emulate.cpp walks the group loads of the unit kernel's surface instantiation over the units the plan compiler
    makes of real tables -- the oracle's tables of BASELINE config 3 direct and blend and of the small rig -- for the pitches FW, FW + 4 and
    a multiple of 256: (a) every dword of every load lies inside the plane of its descriptor or is out of the descriptor's range as a
    whole -- none straddles the end of a plane into foreign memory; (b) what lands in the patch equals what the packed translation lands
    for the same frames; (c) two-camera units fetch every group from the camera the BGR list names;
  * the translation of a group list (bevw_unit.h: unit_gsrc_surf) is exercised through the same program;
  * the Python-level argument checks that need no device, the layout helper of the GPU tests, and the C-ABI additions."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from conftest import ROOT
from oracle import oracle as O
from tests import _nv12_surfaces as SF
from tests._harness import SMALL_CFG, small_rig

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests import _native_build

    path = str(tmp_path_factory.mktemp("nv12surf") / "nv12_surf_emulate")
    _native_build.build(os.path.join(ROOT, "tests", "native", "nv12_surf_emulate.cpp"), path)
    return path


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """The oracle's tables of a rig, written once per rig and mode in the emulator's input format."""
    O.build()
    d = tmp_path_factory.mktemp("nv12surf_tables")
    made = {}

    def get(name, cfg, rig, blend):
        if name not in made:
            gen = O.RefBevGenerator(rig(), cfg, blend=blend, balance=False)
            path = str(d / (name + ".bin"))
            with open(path, "wb") as f:
                f.write(struct.pack("<8i", cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], 4, 0, 0, 0))
                for cam, m in zip(gen.cameras, gen.masks):
                    m1, m2 = cam.bev_maps
                    m = m[..., 0] if m.ndim == 3 else m
                    f.write(np.ascontiguousarray(m1, np.int16).tobytes())
                    f.write(np.ascontiguousarray(m2, np.uint16).tobytes())
                    f.write(np.ascontiguousarray(m, np.uint8).tobytes())
            made[name] = path
        return made[name]

    return get


@needs_hipcc
@pytest.mark.parametrize("pitch", ["fw", "fw+4", "256s"])
@pytest.mark.parametrize("name,cfg,rig,blend", [
    ("config3_direct", W.CONFIG_S, W.rig_s, False),
    ("config3_blend", W.CONFIG_S, W.rig_s, True),
    ("small_blend", SMALL_CFG, small_rig, True),
])
def test_group_loads_of_real_plans(exe, tables, name, cfg, rig, blend, pitch):
    fw = cfg["FRAME_WIDTH"]
    p = {"fw": fw, "fw+4": fw + 4, "256s": (fw + 255) // 256 * 256 + 256}[pitch]
    r = subprocess.run([exe, tables(name, cfg, rig, blend), str(p)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    n = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout)}
    assert n["pitch"] == p and n["groups"] > 10000 and n["dwords_inside"] >= 2 * n["groups"]
    # the rigs have seams: units that sample two cameras exist, and the load instruction that holds the boundary is walked
    assert n["two_camera_units"] > 0 and n["mixed_rounds"] > 0
    assert n["mixed_rounds"] <= 4 * n["two_camera_units"] + n["units"]   # about one per camera boundary: nothing like every round


def test_layout_helper_places_every_plane_inside_the_arena():
    rng = np.random.default_rng(0)
    fw, fh, pitch, n = 16, 8, 24, 6
    frames = rng.integers(0, 256, (n, fh * 3 // 2, fw), dtype=np.uint8)
    for mode in ("shuffled", "split", "packed"):
        y_off, uv_off, size = SF.layout(n, fh, pitch, np.random.default_rng(3), mode)
        arena = np.full(size, 0xEE, np.uint8)
        SF.fill(arena, frames, fw, fh, pitch, y_off, uv_off)
        ysz, csz = SF.plane_sizes(fh, pitch)
        spans = sorted([(int(o), int(o) + ysz) for o in y_off] + [(int(o), int(o) + csz) for o in uv_off])
        assert spans[0][0] >= SF.MARGIN and spans[-1][1] <= size - SF.MARGIN
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "planes overlap"
        assert (y_off % 4 == 0).all() and (uv_off % 4 == 0).all()
        for k in range(n):
            assert np.array_equal(arena[y_off[k]:y_off[k] + ysz].reshape(fh, pitch)[:, :fw], frames[k, :fh])
            assert np.array_equal(arena[uv_off[k]:uv_off[k] + csz].reshape(fh // 2, pitch)[:, :fw], frames[k, fh:])
            assert (arena[y_off[k]:y_off[k] + ysz].reshape(fh, pitch)[:, fw:] == 0xEE).all()   # padding columns untouched
        if mode == "split":
            d = uv_off - y_off
            assert len(set(d.tolist())) == n and (d < 0).any() and (d > 0).any()
        if mode == "packed":
            assert (uv_off - y_off == ysz).all()


def test_python_argument_checks_without_a_device():
    from cameracalibration_amd import _ffi

    assert _ffi.check_input_pitch(None, 1280, True) == 0 and _ffi.check_input_pitch(0, 1280, False) == 0
    assert _ffi.check_input_pitch(1536, 1280, True) == 1536 and _ffi.check_input_pitch(1280, 1280, True) == 1280
    with pytest.raises(Exception, match="input_format='nv12'"):
        _ffi.check_input_pitch(1536, 1280, False)
    for bad in (1276, 1282, 2):
        with pytest.raises(Exception, match="multiple of 4 bytes >= the frame width 1280"):
            _ffi.check_input_pitch(bad, 1280, True)
    t = np.zeros((3, 4, 2), np.uint64)
    assert _ffi.surface_table(t, 4).shape == (3, 4, 2) and _ffi.surface_table(t[:, 0], 1).shape == (3, 2)
    for bad in (t.astype(np.int64), t[:, :3], t[0], np.zeros((3, 4, 3), np.uint64)):
        with pytest.raises(Exception, match=r"uint64 \[B, 4, 2\]"):
            _ffi.surface_table(bad, 4)
    with pytest.raises(Exception, match=r"uint64 \[B, 2\]"):
        _ffi.surface_table(t, 1)
    assert _ffi.surface_table(np.asfortranarray(t), 4).flags["C_CONTIGUOUS"]
    # the keyword is checked before any device call
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB
    from cameracalibration_amd.Tools import undistort as U

    with pytest.raises(Exception, match="input_format='nv12'"):
        SB.BevGenerator(rig=W.repo_rig(), input_pitch=2048)
    with pytest.raises(Exception, match="multiple of 4"):
        SB.BevGenerator(rig=W.repo_rig(), input_format="nv12", input_pitch=SB.BevGenerator.get_args().FRAME_WIDTH + 2)
    K, D = W.undistort_calibration()
    with pytest.raises(Exception, match="input_format='nv12'"):
        U.Undistorter(K, D, 64, 48, input_pitch=128)
    with pytest.raises(Exception, match="multiple of 4"):
        U.Undistorter(K, D, 64, 48, input_format="nv12", input_pitch=60)


def test_abi_additions():
    from cameracalibration_amd import _ffi, build

    build.build()
    L = _ffi.lib()
    assert _ffi.ABI_VERSION == 8 == L.bevw_abi_version()
    for name in ("bevw_set_input_pitch", "bevw_input_pitch", "bevw_run_surfaces_device", "bevw_run_surface_table_device",
                 "bevw_remapper_set_input_pitch", "bevw_remap_surfaces_device", "bevw_remap_surface_table_device"):
        assert name in _ffi.SIGNATURES and hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "bevwarp.h")).read()
    assert re.search(r"typedef struct bevw_nv12_surface \{[^}]*const void \*y;[^}]*const void \*uv;[^}]*\} bevw_nv12_surface;", text, flags=re.S)
    assert "#define BEVW_ABI_VERSION 8" in text
    # null handles are refused before anything touches a device
    assert L.bevw_set_input_pitch(None, 512) == -1 and L.bevw_input_pitch(None) == -1
    assert L.bevw_run_surfaces_device(None, None, 1, None, None) == -1 and L.bevw_run_surface_table_device(None, None, 1, None, None) == -1
    assert L.bevw_remapper_set_input_pitch(None, 512) == -1 and L.bevw_remap_surfaces_device(None, None, 1, None) == -1 and L.bevw_remap_surface_table_device(None, None, 1, None) == -1


@needs_hipcc
def test_surface_kernels_have_names_of_their_own(tmp_path):
    """k_units_surf / k_units_out_surf live in the plan's translation unit beside the four k_plan_units instantiations, and the surface
    instantiations of the per-pixel, remap and V-sum kernels in the library's main unit."""
    from cameracalibration_amd import build
    from tests import _native_build as TU

    build.build()
    plan = TU.kernels_of(os.path.join(build.OBJ, "bevwarp_plan.o"), str(tmp_path))
    main = TU.kernels_of(os.path.join(build.OBJ, "bevwarp.o"), str(tmp_path))
    assert len({k for k in plan if "k_units_surf" in k}) == 2 and len({k for k in plan if "k_units_out_surf" in k}) == 2
    assert len({k for k in plan if "k_plan_units" in k}) == 4
    assert not {k for k in main if "k_units" in k}
    # the layout argument is kLayoutSurf (SrcLayout 2): ...LNS_9SrcLayoutE2E... in the mangled name
    surf = "LNS_9SrcLayoutE2E"
    assert {k for k in main if "k_stitch_pp" in k and surf in k}
    assert {k for k in main if "k_remap_lut" in k and surf in k} and {k for k in main if "k_vsum" in k and surf in k}


@needs_hipcc
def test_surface_table_is_read_with_scalar_loads(tmp_path):
    """The plane pointers reach the unit kernel through s_load_dwordx4 (constant address space, wave-uniform index), not through a vector
    load whose s_waitcnt vmcnt(0) would drain the group loads in flight: the surface kernels hold more scalar 16-byte loads than their
    packed twin and not one more vector global load or v_readfirstlane."""
    from cameracalibration_amd import build
    from tests import _native_build as TU

    build.build()
    TU.kernels_of(os.path.join(build.OBJ, "bevwarp_plan.o"), str(tmp_path))
    dis = subprocess.run([os.path.join(TU.LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", str(tmp_path / "bevwarp_plan.o.co")],
                         check=True, capture_output=True, text=True, timeout=600).stdout
    count = {}
    cur = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if "k_units" in m.group(1):
                cur = m.group(1)
                count[cur] = {"s_load_dwordx4": 0, "global_load": 0, "v_readfirstlane": 0, "flat_load": 0, "scratch_": 0}
            elif not m.group(1).startswith(("L", ".L", "$")) and "BB" not in m.group(1):
                cur = None
            continue
        if cur:
            for k in count[cur]:
                if re.search(r"\s%s" % k, line):
                    count[cur][k] += 1
    packed = {k: v for k, v in count.items() if "k_units_nv12" in k}
    surf = {k: v for k, v in count.items() if "k_units_surf" in k or "k_units_out_surf" in k}
    assert len(packed) == 2 and len(surf) == 4, sorted(count)
    ref = max(packed.values(), key=lambda v: v["global_load"])
    for name, c in surf.items():
        assert c["s_load_dwordx4"] >= ref["s_load_dwordx4"] + 16, (name, c)        # two per frame issue, in every class of the launch
        assert c["global_load"] <= ref["global_load"] and c["v_readfirstlane"] <= ref["v_readfirstlane"], (name, c, ref)
        assert c["flat_load"] == 0 and c["scratch_"] == 0, (name, c)
