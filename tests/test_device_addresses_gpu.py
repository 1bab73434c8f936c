"""The device-resident entry points on buffers at odd ADDRESSES (tests/_device_addresses.py has the catalogue and the rule): d_frames, d_car,
d_out of bevw_run_device and the surface entry, d_src / d_dst of bevw_remap_device, d_out with pitched rows of bevw_jpeg_decode_run_device
and d_bgr of bevw_jpeg_encode_run_device, 1 to 3 bytes off a 4-byte boundary and, for the inputs, 4, 8 and 12 bytes off a 16-byte one.

Every step runs inside arenas filled with 0x5A and asserts, in this order: the PATH the library took (bevw_last_path /
bevw_remapper_last_path: an odd address must land on the per-pixel kernels, the aligned control before AND after it on the units, a pitched
handle must refuse it with nothing written), the fill in front of the buffer and behind its last image, and every image against the CPU
oracle (oracle.RefBevGenerator, oracle.remap; Pillow's libjpeg-turbo for JPEG) at tolerance 0 -- the expected bytes do not depend on where
the caller's buffers lie.  One handle per catalogue entry serves all of its steps.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from tests import _caller_maps as CM
from tests import _device_addresses as DA
from tests import _jpeg_common as JC
from tests import _nv12_out_spec as SO
from tests import _nv12_surfaces as SF
from tests._harness import (FILL, SB, Expected, Remapper, assert_equal, check_image, ffi, generator, image_of, small_rig)  # noqa: F401

pytestmark = pytest.mark.gpu

HANDLES = DA.stitch_handles()
RHANDLES = DA.remap_handles()


# ---------------------------------------------------------------------------------------------------------------
# the stitch handle
# ---------------------------------------------------------------------------------------------------------------
_expected = {}


def expected(oracle, h):
    """(bgr [3], nv12 [3] or None, none) of a handle's frames, car and mode: the oracle's images, computed once and left unchanged."""
    key = (h.cfg, h.inp, h.with_car)
    if key not in _expected:
        _expected[key] = Expected(oracle, DA.content(h.inp)[1], DA.car(h.cfg) if h.with_car else None, DA.CFGS[h.cfg], DA.BATCH, nv12=h.cfg == "small")
    return _expected[key](*DA.MODES[h.mode])


@pytest.mark.parametrize("h", HANDLES, ids=[h.name for h in HANDLES])
def test_stitch_handle(ffi, SB, oracle, h):
    cfg = DA.CFGS[h.cfg]
    bw, bh, fw, fh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    blend, balance = DA.MODES[h.mode]
    want_bgr, want_nv12, none = expected(oracle, h)
    native = DA.content(h.inp)[0]
    car = DA.car(h.cfg) if h.with_car else None
    kw = dict(blend=blend, balance=balance, input_format=h.inp, output_format=h.out, output_pitch=h.pitch,
              schedule=ffi.SCHED_PER_PIXEL if h.schedule == "per_pixel" else ffi.SCHED_TILE_PLAN)
    if h.surfaces:
        kw["input_pitch"] = fw + 4
    bev = generator(SB, small_rig(), cfg, **kw)
    info = bev.plan_info()
    assert info["schedule"] == kw["schedule"] and (h.schedule == "per_pixel" or info["tiles_staged"] > 0), h.name
    assert bev.out_pitch == (256 if h.pitch == "aligned" else bw) and bev.last_path() == ffi.PATH_NONE
    paths = {DA.UNITS: ffi.PATH_UNITS, DA.PER_PIXEL: ffi.PATH_PER_PIXEL}
    nv12, out_bytes = h.out == "nv12", DA.BATCH * bev.out_image_bytes
    a_out, a_car = DA.Arena(ffi, out_bytes), DA.Arena(ffi, car.nbytes) if h.with_car else None
    a_in = surf = d_table = None
    try:
        if h.surfaces:
            surf = SF.Surfaces(ffi, native.reshape(-1, fh * 3 // 2, fw), fw, fh, fw + 4, layout_seed=161, fill_seed=162, mode="shuffled")
            d_table = ffi.DeviceBuffer(surf.table.nbytes).upload(surf.table)
        else:
            assert bev.in_set_bytes * DA.BATCH == native.nbytes
            a_in = DA.Arena(ffi, native.nbytes)
        for s in h.steps:
            before = bev.last_path()
            p_car = a_car.place(car, s.car) if h.with_car else None
            p_out = a_out.clear(s.out)
            if h.surfaces:
                run = lambda: bev.run_surface_table(d_table.ptr, DA.BATCH, p_car, p_out, out_bytes=out_bytes)
            else:
                p_in = a_in.place(native, s.frames)
                run = lambda: bev.run_device(p_in, DA.BATCH, p_car, p_out, out_bytes=out_bytes)
            if s.expect == DA.REFUSE:
                with pytest.raises(ffi.BevwError, match="4-byte aligned"):
                    run()
                bev.sync()
                a_out.untouched(s.name)
                assert bev.last_path() == before, s.name
                continue
            run()
            bev.sync()
            assert bev.last_path() == paths[s.expect], "%s: path %d, expected %d (%s)" % (s.name, bev.last_path(), paths[s.expect], s.expect)
            raw = a_out.read(s.out, out_bytes, s.name).reshape(DA.BATCH, bev.out_image_bytes)
            for b in range(DA.BATCH):
                check_image(image_of(raw[b], nv12, bw, bh, bev.out_pitch), want_bgr[b], none, "%s, image %d" % (s.name, b), h.out, car=car,
                            want_nv12=want_nv12[b] if nv12 else None)
    finally:
        for a in (a_out, a_car, a_in, d_table, surf):
            if a is not None:
                a.free()


def test_last_path_of_the_analytic_projection(ffi, SB):
    """bevw_last_path where stitch_analytic decides: the wide unit plan on aligned buffers, the full-grid kernel for d_out + 1 and for a
    balance handle.  Only the path: the images of these steps are tests/test_analytic_gpu.py's (the analytic projection at odd addresses
    is covered there)."""
    cfg, native, car = DA.CFGS["small"], DA.content("bgr")[0], DA.car("small")
    for balance, expect in ((False, (ffi.PATH_UNITS, ffi.PATH_PER_PIXEL, ffi.PATH_UNITS)), (True, (ffi.PATH_PER_PIXEL,) * 3)):
        bev = generator(SB, small_rig(), cfg, blend=True, balance=balance, projection="analytic")
        out_bytes = DA.BATCH * bev.out_image_bytes
        a_in, a_car, a_out = DA.Arena(ffi, native.nbytes), DA.Arena(ffi, car.nbytes), DA.Arena(ffi, out_bytes)
        try:
            assert bev.out_pitch == cfg["BEV_WIDTH"] and bev.last_path() == ffi.PATH_NONE
            for off, path in zip((0, 1, 0), expect):
                bev.run_device(a_in.place(native, 0), DA.BATCH, a_car.place(car, 0), a_out.clear(off), out_bytes=out_bytes)
                bev.sync()
                assert bev.last_path() == path, "analytic, balance %d, d_out + %d: path %d, expected %d" % (balance, off, bev.last_path(), path)
                a_out.read(off, out_bytes, "analytic, balance %d, d_out + %d" % (balance, off))
        finally:
            for a in (a_in, a_car, a_out):
                a.free()


# ---------------------------------------------------------------------------------------------------------------
# the three-channel remapper
# ---------------------------------------------------------------------------------------------------------------
_maps, _remapped = {}, {}


def maps_of(oracle, name):
    """-> (map1, map2), (sw, sh, dw, dh)"""
    if name not in _maps:
        if name == "undistort_front":
            cfg = DA.CFGS["small"]
            fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
            K, D, _ = small_rig()["front"]
            size = (int(fw * cfg["SIZE_SCALE"]), int(fh * cfg["SIZE_SCALE"]))
            m = oracle.fisheye_init_undistort_rectify_map(K, D, oracle.camera_mat_dst(K, fw, fh, cfg["FOCAL_SCALE"], cfg["SIZE_SCALE"]), size)
            _maps[name] = ((np.ascontiguousarray(m[0]), np.ascontiguousarray(m[1])), (fw, fh) + size)
        else:
            _maps[name] = (CM.family(name, *CM.SMALL), CM.SMALL)
    return _maps[name]


def remapped(oracle, name, inp, out):
    key = (name, inp)
    if key not in _remapped:
        (m1, m2), size = maps_of(oracle, name)
        _remapped[key] = np.stack([oracle.remap(f, m1, m2) for f in DA.remap_frames(size[0], size[1], inp)[1]])
        _remapped[key].setflags(write=False)
    return SO.bgr_to_nv12(_remapped[key]) if out == "nv12" else _remapped[key]


@pytest.mark.parametrize("h", RHANDLES, ids=[h.name for h in RHANDLES])
def test_remapper(ffi, oracle, h):
    maps, size = maps_of(oracle, h.maps)
    raw = DA.remap_frames(size[0], size[1], h.inp)[0]
    want = remapped(oracle, h.maps, h.inp, h.out)
    paths = {DA.UNITS: ffi.PATH_UNITS, DA.PER_PIXEL: ffi.PATH_PER_PIXEL}
    a_src, a_dst = DA.Arena(ffi, raw.nbytes), DA.Arena(ffi, want.nbytes)
    try:
        with Remapper(ffi, maps, size, h.inp) as r:
            r.set_output(h.out)
            assert r.out_shape(h.out, DA.BATCH) == want.shape and r.last_path() == ffi.PATH_NONE
            for s in h.steps:
                r.remap_device(a_src.place(raw, s.src), DA.BATCH, a_dst.clear(s.dst))
                assert r.last_path() == paths[s.expect], "%s: path %d, expected %d (%s)" % (s.name, r.last_path(), paths[s.expect], s.expect)
                got = a_dst.read(s.dst, want.nbytes, s.name).reshape(want.shape)
                for b in range(DA.BATCH):
                    assert_equal(got[b], want[b], "%s, image %d" % (s.name, b))
    finally:
        a_src.free()
        a_dst.free()


# ---------------------------------------------------------------------------------------------------------------
# JPEG: Pillow's libjpeg-turbo is the reference, as in tests/test_jpeg_gpu.py
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec(ffi):
    pytest.importorskip("PIL")
    from cameracalibration_amd import imgcodecs

    c = imgcodecs.JpegCodec(0)
    yield c
    c.close()


@pytest.mark.parametrize("sub,code", DA.JPEG_SUBSAMPLINGS)
@pytest.mark.parametrize("h,w", DA.JPEG_SIZES)
def test_jpeg_decode_into_pitched_rows_at_any_address(ffi, codec, h, w, sub, code):
    files = [JC.pil_encode(im, 90, code) for im in DA.jpeg_images(h, w)]
    want = [JC.pil_decode(f) for f in files]
    n = len(files)
    cases = DA.decode_cases(h, w, sub)
    arena = DA.Arena(ffi, n * max(c.stride for c in cases))
    try:
        for c in cases:
            codec.decode_stage(files)
            codec.decode_run_device(arena.clear(c.off), c.stride, c.pitch)
            codec.sync()
            assert codec.decode_info()["short_images"] == 0, c.name
            raw = arena.read(c.off, n * c.stride, c.name).reshape(n, c.stride)
            for i in range(n):
                rows, gap = raw[i, :c.pitch * h].reshape(h, c.pitch), raw[i, c.pitch * h:]
                assert_equal(rows[:, :w * 3].reshape(h, w, 3), want[i], "%s, image %d" % (c.name, i))
                assert (rows[:, w * 3:] == FILL).all(), "%s, image %d: %d bytes of the padding columns were written" % (
                    c.name, i, int((rows[:, w * 3:] != FILL).sum()))
                assert (gap == FILL).all(), "%s: %d bytes of the gap behind image %d were written" % (c.name, int((gap != FILL).sum()), i)
    finally:
        arena.free()


@pytest.mark.parametrize("h,w", DA.JPEG_SIZES)
def test_jpeg_encode_from_pitched_rows_at_odd_addresses(ffi, codec, h, w):
    ims = DA.jpeg_images(h, w)
    want = [JC.pil_encode(im) for im in ims]
    n = len(want)
    cases = DA.encode_cases(h, w)
    arena = DA.Arena(ffi, n * max(c.stride for c in cases))
    try:
        for c in cases:
            src = np.full((n, c.stride), DA.ENCODE_PADDING, np.uint8)   # padding columns and gaps must not leak into the file
            for i in range(n):
                src[i, :c.pitch * h].reshape(h, c.pitch)[:, :w * 3] = ims[i].reshape(h, w * 3)
            codec.encode_run_device(arena.place(src, c.off), n, w, h, c.stride, c.pitch)
            got = codec.files()
            for i in range(n):
                assert got[i] == want[i], "%s, image %d: the file differs from libjpeg-turbo's (%d bytes against %d)" % (c.name, i, len(got[i]), len(want[i]))
    finally:
        arena.free()
