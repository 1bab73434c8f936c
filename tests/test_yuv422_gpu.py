"""Packed 4:2:2 camera frames (bevw_set_input_format: YUYV / UYVY; BevGenerator(input_format='yuyv' | 'uyvy'), Undistorter(input_format=...))
on the GPU.

The reference result is always the CPU oracle (oracle.RefBevGenerator, oracle.remap) applied to the BGR frames the NumPy specification
(tests/_yuv422_spec.py: cv2.cvtColor(f, cv2.COLOR_YUV2BGR_YUY2 / COLOR_YUV2BGR_UYVY)) makes of the input, compared with tolerance 0; NV12
output is compared with tests/_nv12_out_spec applied to the oracle's BGR.  Pixels no camera covers are asserted on their own first, and
must exist: a kernel that lets the conversion of YUV (0, 0, 0) = (B, G, R) (0, 154, 0) into a tap without a texel fails there by name.

The unit classes a plan populates are not part of the public diagnostics.  The plan of a handle does not depend on its input format (the
group lists alone are translated), so section 3 asserts that the 4:2:2 handle's plan_info() is the BGR handle's: every class the BGR
plan runs is run, on the geometry where the 1024-group classes exist.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests import _nv12_out_spec as SO
from tests import _yuv422_spec as S
from tests._harness import SMALL_CFG, SB, assert_nv12, assert_same, check_image, ffi, generator, random_car, raw_handle, small_rig, uncovered  # noqa: F401

pytestmark = pytest.mark.gpu
E_INVALID = -1


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's generators, built once per (rig, blend, balance), with the pixels no camera covers."""
    made = {}

    def get(name, blend, balance):
        key = (name, bool(blend), bool(balance))
        if key not in made:
            rig, cfg = (small_rig(), SMALL_CFG) if name == "small" else (W.rig_s(), W.CONFIG_S)
            ref = oracle.RefBevGenerator(rig, cfg, blend=blend, balance=balance)
            none = uncovered(ref)
            assert none.any(), "the rig has pixels no camera covers"
            made[key] = (ref, none)
        return made[key]

    return get


# ---------------------------------------------------------------------------------------------------------------
# 1. small rig: both byte orders, every mode, both schedules, BGR and NV12 images, random frames and a random car
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("sched", ["auto", "per_pixel"])
@pytest.mark.parametrize("blend,balance", [(False, False), (True, False), (True, True)], ids=["direct", "blend", "blend_balance"])
@pytest.mark.parametrize("order", S.ORDERS)
def test_small_rig_matches_oracle_on_converted_frames(ffi, SB, refs, order, blend, balance, sched, out, pitch="auto"):
    cfg = SMALL_CFG
    rng = np.random.default_rng(4220 + 16 * (order == "uyvy") + 8 * blend + 4 * balance + 2 * (sched == "auto") + (out == "nv12"))
    schedule = ffi.SCHED_PER_PIXEL if sched == "per_pixel" else ffi.SCHED_AUTO
    bev = generator(SB, small_rig(), cfg, blend=blend, balance=balance, schedule=schedule, output_pitch=pitch, input_format=order, output_format=out)
    assert ffi.lib().bevw_input_format(bev._engine.h) == ffi.INPUT_FORMATS[order]
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    assert bev.in_set_bytes == 4 * fw * fh * 2
    if sched == "auto":
        info = bev.plan_info()
        assert info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0   # the unit kernel's 4:2:2 instantiation runs
    ref, none = refs("small", blend, balance)
    car = random_car(rng, cfg)
    frames = S.random_yuv422(rng, (3, 4), fw, fh)
    bgr = S.yuv422_to_bgr(frames, order)
    got = bev.batch(frames, car)
    for b in range(3):
        check_image(got[b], ref(*bgr[b], car), none, "set %d" % b, out, black=False)
    assert np.array_equal(bev(*frames[0], car), got[0])


@pytest.mark.parametrize("out", ["bgr", "nv12"])
def test_small_rig_dense_pitch(ffi, SB, refs, out):
    test_small_rig_matches_oracle_on_converted_frames(ffi, SB, refs, "yuyv", True, False, "auto", out, pitch="dense")


def test_odd_height_and_width_no_multiple_of_4(ffi, SB, oracle):
    """322 x 255 frames, blend + balance: an odd height (legal: chroma is shared inside a row only), rows that are not whole 4-texel groups
    (no unit plan: the per-tap kernel serves every tile, with the luminance round trip) and frames of 322 * 255 * 2 bytes, no multiple
    of 16 (the V sums take their byte path)."""
    cfg = dict(SMALL_CFG, FRAME_WIDTH=322, FRAME_HEIGHT=255)
    rng = np.random.default_rng(322255)
    bev = generator(SB, small_rig(), cfg, blend=True, balance=True, input_format="uyvy")
    assert bev.plan_info()["tiles_staged"] == 0
    ref = oracle.RefBevGenerator(small_rig(), cfg, blend=True, balance=True)
    none = uncovered(ref)
    assert none.any()
    car = random_car(rng, cfg)
    frames = S.random_yuv422(rng, (2, 4), 322, 255)
    got = bev.batch(frames, car)
    for b in range(2):
        assert_same(got[b], ref(*S.yuv422_to_bgr(frames[b], "uyvy"), car), none, "set %d" % b)


# ---------------------------------------------------------------------------------------------------------------
# 2. a batch that is no multiple of its chunks, through run_device: the prefetch ring of the last block runs past the chunk's end
#    (the last frame once more), and the descriptor of the batch's last set ends where the buffer ends
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_ragged_batch_run_device(ffi, SB, refs, blend):
    cfg = SMALL_CFG
    fw, fh, bw, bh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    batch = 19
    rng = np.random.default_rng(190 + blend)
    frames = S.random_yuv422(rng, (batch, 4), fw, fh)
    bev = generator(SB, small_rig(), cfg, blend=blend, input_format="yuyv")
    assert bev.plan_info()["tiles_staged"] > 0
    ref, none = refs("small", blend, False)
    d_in = ffi.DeviceBuffer(frames.nbytes).upload(frames)   # exactly batch * in_set_bytes: nothing behind the last set
    d_out = ffi.DeviceBuffer(batch * bev.out_image_bytes)
    try:
        assert frames.nbytes == batch * bev.in_set_bytes
        bev.run_device(d_in.ptr, batch, None, d_out.ptr, out_bytes=d_out.nbytes)
        bev.sync()
        for b in (0, 15, 16, 18):
            got = d_out.download((bh, bev.out_pitch, 3), offset=b * bev.out_image_bytes)[:, :bw]
            assert_same(got, ref(*S.yuv422_to_bgr(frames[b], "yuyv")), none, "set %d of %d" % (b, batch))
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 3. BASELINE config 3 / config 4 geometry (where every unit class is populated), batch 2 through run_device, pitched
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,out", [("yuyv", "bgr"), ("uyvy", "nv12")])
@pytest.mark.parametrize("blend,balance", [(False, False), (True, True)], ids=["config3", "config4"])
def test_baseline_geometry_every_unit_class(ffi, SB, refs, blend, balance, order, out):
    cfg = W.CONFIG_S
    fw, fh, bw, bh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    rng = np.random.default_rng(340 + 2 * blend + (out == "nv12"))
    frames = S.random_yuv422(rng, (2, 4), fw, fh)
    bev = generator(SB, W.rig_s(), cfg, blend=blend, balance=balance, output_pitch="auto", input_format=order, output_format=out)
    plain = generator(SB, W.rig_s(), cfg, blend=blend, balance=balance, output_pitch="auto", output_format=out)
    info = bev.plan_info()
    assert info == plain.plan_info() and info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0   # the BGR handle's plan, unit for unit
    assert bev.out_pitch != bw or bw % 16 == 0
    ref, none = refs("config_s", blend, balance)
    d_in = ffi.DeviceBuffer(frames.nbytes).upload(frames)
    d_out = ffi.DeviceBuffer(2 * bev.out_image_bytes)
    try:
        bev.run_device(d_in.ptr, 2, None, d_out.ptr, out_bytes=d_out.nbytes)
        bev.sync()
        for b in range(2):
            want = ref(*S.yuv422_to_bgr(frames[b], order))
            if out == "nv12":
                raw = d_out.download((bev.out_image_bytes,), offset=b * bev.out_image_bytes)
                assert_nv12(SO.from_device(raw, bw, bh, bev.out_pitch), want, none, "set %d" % b)
            else:
                got = d_out.download((bh, bev.out_pitch, 3), offset=b * bev.out_image_bytes)[:, :bw]
                assert_same(got, want, none, "set %d" % b)
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 4. undistort: the unit plan, the ties-to-even per-pixel kernel, and a source the remapper serves without units
# ---------------------------------------------------------------------------------------------------------------
def run_undistort(ffi, oracle, w, h, batch, order, ties_even, out, seed):
    from cameracalibration_amd.Tools import undistort as U

    cfg = W.CONFIG_UNDISTORT
    K, D = W.undistort_calibration()
    s = w / float(cfg["FRAME_WIDTH"])
    K = np.diag([s, s, 1.0]) @ np.asarray(K, np.float64).reshape(3, 3)   # the calibration scaled to the source size
    L = ffi.lib()
    rng = np.random.default_rng(seed)
    imgs = S.random_yuv422(rng, (batch,), w, h)
    bgr = S.yuv422_to_bgr(imgs, order)
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, ties_even))
        oracle.set_variant(oracle.VARIANT_REMAP, ties_even)
        und = U.Undistorter(K, D, w, h, focalscale=cfg["FOCAL_SCALE"], sizescale=cfg["SIZE_SCALE"], input_format=order, output_format=out)
        got = und(imgs)
        one = und(imgs[batch - 1])
        m1, m2 = und.maps()
        Kd = oracle.camera_mat_dst(K, w, h, cfg["FOCAL_SCALE"], cfg["SIZE_SCALE"])
        o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, (und.out_w, und.out_h))
        assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
        outside = (o1[..., 0] < -1) | (o1[..., 0] >= w) | (o1[..., 1] < -1) | (o1[..., 1] >= h)
        for b in range(batch):
            check_image(got[b], oracle.remap(bgr[b], o1, o2), outside, "image %d" % b, out, black=True)
        assert np.array_equal(one, got[batch - 1])
        und.close()
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)
        oracle.set_variant(oracle.VARIANT_REMAP, 0)


@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("ties_even", [0, 1])
@pytest.mark.parametrize("order", S.ORDERS)
def test_undistort(ffi, oracle, order, ties_even, out):
    run_undistort(ffi, oracle, 320, 256, 5, order, ties_even, out, 500 + 4 * (order == "uyvy") + 2 * ties_even + (out == "nv12"))


def test_undistort_source_width_no_multiple_of_4(ffi, oracle):
    """66 x 48: even, so a legal 4:2:2 frame, but no unit plan (rows are not whole 4-texel groups): the per-tap kernel serves every tile."""
    run_undistort(ffi, oracle, 66, 48, 3, "uyvy", 0, "bgr", 66)


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals and shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", S.ORDERS)
def test_refusals(ffi, SB, order):
    L = ffi.lib()
    fmt = ffi.INPUT_FORMATS[order]
    name = order.upper().encode()
    # analytic projection, in both orders
    with pytest.raises(ffi.BevwError, match="analytic"):
        generator(SB, small_rig(), SMALL_CFG, projection="analytic", input_format=order)
    bev = generator(SB, small_rig(), SMALL_CFG, projection="analytic_f32")
    assert L.bevw_set_input_format(bev._engine.h, fmt) == E_INVALID and b"analytic" in L.bevw_last_error()
    # camera-shard handles, in both orders; the values that are no formats; the round trip
    h = raw_handle(ffi, 320, 256, 248, 250)
    try:
        ffi.check(L.bevw_set_input_format(h, fmt))
        assert L.bevw_input_format(h) == fmt
        cams = (C.c_int32 * 2)(0, 2)
        assert L.bevw_set_camera_shard(h, cams, 2) == E_INVALID and name in L.bevw_last_error()
        assert L.bevw_set_projection(h, ffi.PROJ_ANALYTIC) == E_INVALID and name in L.bevw_last_error()
        assert L.bevw_set_input_pitch(h, 512) == E_INVALID and b"NV12" in L.bevw_last_error()
        for bad in (2, 3, -1, 6):
            assert L.bevw_set_input_format(h, bad) == E_INVALID
        assert L.bevw_input_format(h) == fmt
        ffi.check(L.bevw_set_input_format(h, ffi.INPUT_BGR))
        assert L.bevw_input_format(h) == ffi.INPUT_BGR
        ffi.check(L.bevw_set_camera_shard(h, cams, 2))
        assert L.bevw_set_input_format(h, fmt) == E_INVALID and b"shard" in L.bevw_last_error()
    finally:
        L.bevw_destroy(h)
    # an odd frame width is refused, an odd height is not
    h = raw_handle(ffi, 321, 256, 248, 250)
    try:
        assert L.bevw_set_input_format(h, fmt) == E_INVALID and b"even" in L.bevw_last_error()
    finally:
        L.bevw_destroy(h)
    h = raw_handle(ffi, 320, 257, 248, 250)
    try:
        ffi.check(L.bevw_set_input_format(h, fmt))
    finally:
        L.bevw_destroy(h)
    rng = np.random.default_rng(5)
    m1 = rng.integers(0, 60, (40, 48, 2)).astype(np.int16)
    m2 = rng.integers(0, 1024, (40, 48)).astype(np.uint16)
    r = C.c_void_p()
    ffi.check(L.bevw_remapper_from_maps(0, 63, 64, ffi.ptr(m1), ffi.ptr(m2), 48, 40, C.byref(r)))
    try:
        assert L.bevw_remapper_set_input_format(r, fmt) == E_INVALID and b"even" in L.bevw_last_error()
        assert L.bevw_remapper_set_input_format(r, 2) == E_INVALID and L.bevw_remapper_set_input_format(r, 3) == E_INVALID
    finally:
        L.bevw_remapper_destroy(r)
    # surfaces stay NV12, JPEG entry points decode to BGR; shapes
    gen = generator(SB, small_rig(), SMALL_CFG, input_format=order)
    with pytest.raises(Exception, match="input_format='nv12'"):
        generator(SB, small_rig(), SMALL_CFG, input_format=order, input_pitch=512)
    with pytest.raises(Exception, match="input_format='nv12'"):
        gen.run_surfaces(np.zeros((1, 4, 2), np.uint64), None, 0)
    with pytest.raises(Exception, match="input_format='nv12'"):
        gen.run_surface_table(0, 1, None, 0)
    with pytest.raises(Exception, match="input_format='bgr'"):
        gen.jpeg([[b"", b"", b"", b""]])
    with pytest.raises(Exception, match="input_format='bgr'"):
        list(gen.jpeg_stream([[[b"", b"", b"", b""]]]))
    fw, fh = SMALL_CFG["FRAME_WIDTH"], SMALL_CFG["FRAME_HEIGHT"]
    bgr = np.zeros((fh, fw, 3), np.uint8)
    nv = np.zeros((fh * 3 // 2, fw), np.uint8)
    with pytest.raises(Exception, match=r"\(256, 320, 2\)"):
        gen(bgr, bgr, bgr, bgr)
    with pytest.raises(Exception, match=r"\(256, 320, 2\)"):
        gen(nv, nv, nv, nv)
    with pytest.raises(Exception, match=r"\(256, 320, 2\)"):
        gen(*np.zeros((4, fh, fw, 2), np.float32))
    with pytest.raises(Exception, match=r"\[B, 4, 256, 320, 2\]"):
        gen.batch(np.zeros((1, 4, fh, fw, 3), np.uint8))
    with pytest.raises(Exception, match=r"\[B, 4, 256, 320, 2\]"):
        gen.batch(np.zeros((1, 4, fh * 3 // 2, fw), np.uint8))
    with pytest.raises(Exception, match="bgr/nv12"):
        generator(SB, small_rig(), SMALL_CFG, input_format="yvyu")
    from cameracalibration_amd.Tools import undistort as U

    K, D = W.undistort_calibration()
    und = U.Undistorter(K, D, 64, 48, input_format=order)
    with pytest.raises(Exception, match=r"\[B, 48, 64, 2\]"):
        und(np.zeros((2, 48, 64, 3), np.uint8))
    with pytest.raises(Exception, match="input_format='nv12'"):
        und.run_surfaces(np.zeros((1, 2), np.uint64), 0)
    und.close()
