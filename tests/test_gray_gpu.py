"""Single-channel images through the remapper (bevw_remapper_set_channels, Undistorter(channels=1), InCalibrator.undistort on a [FH, FW]
image) on the GPU: k_units_gray on the unit schedule, k_stitch_plan_gray for the frame-border tiles, k_remap_lut_gray as the fall-back.

The expected value is always oracle.remap on the 2-D array, compared with tolerance 0 over all pixels.  Pixels the map sends wholly outside
the frame are asserted to be 0 on their own first.  Which kernels served a step is asked of the library (bevw_remapper_last_path) and
asserted, so that no case passes through the fall-back unnoticed.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests import _caller_maps as CM
from tests import _gray_maps as GM
from tests._harness import Remapper, assert_batch_gray as assert_batch, assert_same_gray as assert_same, ffi, outside_of, run_child  # noqa: F401

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120   # seconds: a library load and one small remapper take a few seconds
FOCAL_SCALE = 0.1     # the fisheye view zoomed out until its rim leaves the frame (at the benchmark's 0.5 every pixel samples inside)


def gray_frames(sw, sh, n, seed):
    """n frames of uniform random bytes."""
    return np.random.default_rng([seed, sw, sh]).integers(0, 256, (n, sh, sw), dtype=np.uint8)


def want_of(oracle, frames, m1, m2, variant=0):
    before = oracle.get_variant(oracle.VARIANT_REMAP)
    try:
        oracle.set_variant(oracle.VARIANT_REMAP, variant)
        return np.stack([oracle.remap(f, m1, m2) for f in frames])
    finally:
        oracle.set_variant(oracle.VARIANT_REMAP, before)


def replicate(frames):
    return np.ascontiguousarray(np.repeat(frames[..., None], 3, -1))


# ---------------------------------------------------------------------------------------------------------------
# 1. / 2. Undistorter(channels=1): the unit schedule, the ties-to-even per-pixel kernel, a source without a plan
# ---------------------------------------------------------------------------------------------------------------
def run_undistort(ffi, oracle, w, h, batch, ties_even, path, seed):
    from cameracalibration_amd.Tools import undistort as U

    cfg = W.CONFIG_UNDISTORT
    K, D = W.undistort_calibration()
    s = w / float(cfg["FRAME_WIDTH"])
    K = np.diag([s, s, 1.0]) @ np.asarray(K, np.float64).reshape(3, 3)   # the calibration scaled to the source size
    L = ffi.lib()
    imgs = gray_frames(w, h, batch, seed)
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, ties_even))
        oracle.set_variant(oracle.VARIANT_REMAP, ties_even)
        und = U.Undistorter(K, D, w, h, focalscale=FOCAL_SCALE, sizescale=cfg["SIZE_SCALE"], channels=1)
        try:
            assert und.last_path() == ffi.PATH_NONE and und.out_image_bytes == und.out_w * und.out_h
            got = und(imgs)
            assert und.last_path() == path, "path %d, expected %d" % (und.last_path(), path)
            assert got.shape == (batch, und.out_h, und.out_w)
            one = und(imgs[batch - 1])
            assert one.shape == (und.out_h, und.out_w)
            m1, m2 = und.maps()
            Kd = oracle.camera_mat_dst(K, w, h, FOCAL_SCALE, cfg["SIZE_SCALE"])
            o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, (und.out_w, und.out_h))
            assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
            outside = outside_of(o1, w, h)
            assert outside.any()
            for b in range(batch):
                assert_same(got[b], oracle.remap(imgs[b], o1, o2), outside, "image %d" % b)
            assert np.array_equal(one, got[batch - 1])
        finally:
            und.close()
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)
        oracle.set_variant(oracle.VARIANT_REMAP, 0)


@pytest.mark.parametrize("ties_even", [0, 1])
def test_undistort_320x256(ffi, oracle, ties_even):
    run_undistort(ffi, oracle, 320, 256, 5, ties_even, ffi.PATH_PER_PIXEL if ties_even else ffi.PATH_UNITS, 900 + ties_even)


def test_undistort_66x48_has_no_plan(ffi, oracle):
    run_undistort(ffi, oracle, 66, 48, 5, 0, ffi.PATH_PER_PIXEL, 910)   # src_w % 4 != 0


# ---------------------------------------------------------------------------------------------------------------
# 3. caller-made maps: every family at every size of the catalogue, batch 2
# ---------------------------------------------------------------------------------------------------------------
CASES = [(name, size) for name in CM.FAMILIES for size in CM.sizes(name)]
OUTSIDE_FAMILIES = ("scatter", "minify8", "extremes", "strip_w", "strip_h", "strip_w4")   # their definitions put footprints wholly outside the frame
UNIT_FAMILIES = ("transpose", "rot180", "magnify16")   # smooth maps inside the frame: the unit schedule owns them whole (tests/test_gray_host.py)


@pytest.mark.parametrize("name,size", CASES, ids=["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASES])
def test_caller_maps(ffi, oracle, name, size):
    sw, sh, dw, dh = size
    maps = CM.family(name, sw, sh, dw, dh)
    frames = gray_frames(sw, sh, 2, 920 + CM.FAMILIES.index(name))
    outside = outside_of(maps[0], sw, sh)
    if name in OUTSIDE_FAMILIES:
        assert outside.any()
    want = want_of(oracle, frames, *maps)
    with Remapper(ffi, maps, size, channels=1) as g, Remapper(ffi, maps, size, channels=3) as c:
        got = g.remap(frames)
        gray_path = g.last_path()
        c.remap(replicate(frames))
        bgr_path = c.last_path()
    for b in range(2):
        assert_same(got[b], want[b], outside, "%s at %s, image %d" % (name, size, b))
    print("%s %s: grey path %d, BGR path %d" % (name, size, gray_path, bgr_path))
    # the unit schedule wherever the geometry allows it and the plan compiler itself made units for these maps (what the three-channel
    # remapper ran on the same maps says so)
    if sw % 4 == 0 and dw % 4 == 0 and bgr_path == ffi.PATH_UNITS:
        assert gray_path == ffi.PATH_UNITS
    else:
        assert gray_path == ffi.PATH_PER_PIXEL
    if name in UNIT_FAMILIES:
        assert gray_path == ffi.PATH_UNITS


# ---------------------------------------------------------------------------------------------------------------
# 4. ragged batch 19 through bevw_remap_device, device buffers of exactly the batch's bytes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "minify8", "edge_shift"])
def test_ragged_batch_19_on_exact_device_buffers(ffi, oracle, name):
    """19 frames: chunks of 2 and a last chunk of 1, whose frame ring runs past the chunk's end, and a source descriptor that ends where
    the buffer ends.  `corner` samples the last group of the last row of the last frame; every base tile of it is a frame-border tile, so
    the plan compiler makes no unit and the per-pixel kernel serves it.  `minify8` is the unit schedule's case, with units that own nothing
    but pixels outside the frame.  `edge_shift` (tests/_gray_maps.py) is the unit schedule up to the frame's last texel: its units fetch
    the groups next to the last group of the last row, which itself is the per-tap kernel's (tests/test_gray_host.py says why no unit
    load reaches past the frames)."""
    size = CM.SMALL
    sw, sh, dw, dh = size
    maps = GM.edge_shift(sw, sh, dw, dh) if name == "edge_shift" else CM.family(name, sw, sh, dw, dh)
    assert name != "edge_shift" or (maps[0][-1, -1] == (sw - 2, sh - 2)).all()
    assert name != "corner" or (maps[0][..., 0].max() == sw - 1 and maps[0][..., 1].max() == sh - 1)
    frames = gray_frames(sw, sh, 19, 950)
    outside = outside_of(maps[0], sw, sh)
    assert name != "minify8" or outside.any()
    d_in, d_out = ffi.DeviceBuffer(19 * sw * sh).upload(frames), ffi.DeviceBuffer(19 * dw * dh)
    try:
        d_out.fill(0x5a)
        with Remapper(ffi, maps, size, channels=1) as g:
            g.remap_device(d_in.ptr, 19, d_out.ptr)
            path = g.last_path()
        print("%s: path %d" % (name, path))
        assert path == (ffi.PATH_PER_PIXEL if name == "corner" else ffi.PATH_UNITS)
        got = d_out.download((19, dh, dw))
        for b in (0, 15, 16, 18):
            assert_same(got[b], oracle.remap(frames[b], *maps), outside, "%s set %d" % (name, b))
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 5. what sends a step to the per-pixel kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trigger", ["dst_w_158", "src_plus_1", "dst_plus_2"])
def test_fall_back_triggers(ffi, oracle, trigger):
    size = (256, 192, 158, 120) if trigger == "dst_w_158" else CM.SMALL
    sw, sh, dw, dh = size
    maps = CM.family("minify8", sw, sh, dw, dh)
    frames = gray_frames(sw, sh, 3, 960)
    outside = outside_of(maps[0], sw, sh)
    assert outside.any()
    so, do = (1 if trigger == "src_plus_1" else 0), (2 if trigger == "dst_plus_2" else 0)
    d_in, d_out = ffi.DeviceBuffer(frames.nbytes + 4), ffi.DeviceBuffer(3 * dw * dh + 4)
    try:
        d_in.upload(frames, offset=so)
        d_out.fill(0x5a)
        with Remapper(ffi, maps, size, channels=1) as g:
            if trigger != "dst_w_158":   # the same remapper on aligned pointers runs the units: the trigger is the pointer alone
                d_al = ffi.DeviceBuffer(frames.nbytes).upload(frames)
                try:
                    g.remap_device(d_al.ptr, 3, d_out.ptr)
                finally:
                    d_al.free()
                assert g.last_path() == ffi.PATH_UNITS
                d_out.fill(0x5a)
            g.remap_device(d_in.ptr + so, 3, d_out.ptr + do)
            assert g.last_path() == ffi.PATH_PER_PIXEL
        got = d_out.download((3, dh, dw), offset=do)
        for b in range(3):
            assert_same(got[b], oracle.remap(frames[b], *maps), outside, "%s image %d" % (trigger, b))
    finally:
        d_in.free()
        d_out.free()


def test_plan_switched_off(ffi, oracle, tmp_path):
    """BEVW_REMAP_PLAN=0 is read once: a fresh process (tests/_gray_worker.py)."""
    sw, sh, dw, dh = CM.SMALL
    maps = CM.family("minify8", sw, sh, dw, dh)
    frames = gray_frames(sw, sh, 3, 970)
    assert outside_of(maps[0], sw, sh).any()
    case_file = str(tmp_path / "case.npz")
    np.savez(case_file, frames=frames, want=want_of(oracle, frames, *maps))
    run_child("_gray_worker.py", [case_file], {"BEVW_REMAP_PLAN": "0"}, timeout=CHILD_TIMEOUT)


# ---------------------------------------------------------------------------------------------------------------
# 6. / 7. against the three-channel remapper on the device; the setter walk
# ---------------------------------------------------------------------------------------------------------------
def test_gray_equals_a_channel_of_the_bgr_remapper(ffi):
    size = CM.SMALL
    maps = CM.family("swirl", *size)
    frames = gray_frames(size[0], size[1], 4, 980)
    with Remapper(ffi, maps, size, channels=1) as g, Remapper(ffi, maps, size, channels=3) as c:
        got, bgr = g.remap(frames), c.remap(replicate(frames))
        assert g.last_path() == ffi.PATH_UNITS and c.last_path() == ffi.PATH_UNITS
    assert np.array_equal(got, bgr[..., 0]) and np.array_equal(bgr[..., 0], bgr[..., 1]) and np.array_equal(bgr[..., 0], bgr[..., 2])


def test_setter_walk_3_1_3_1(ffi, oracle):
    size = CM.SMALL
    sw, sh = size[:2]
    maps = CM.family("minify8", *size)
    outside = outside_of(maps[0], sw, sh)
    assert outside.any()
    gray = gray_frames(sw, sh, 3, 990)
    bgr = np.random.default_rng(991).integers(0, 256, (3, sh, sw, 3), dtype=np.uint8)
    want_gray = want_of(oracle, gray, *maps)
    want_bgr = want_of(oracle, bgr, *maps)
    with Remapper(ffi, maps, size, channels=3) as never, Remapper(ffi, maps, size, channels=3) as r:
        ref = never.remap(bgr)
        assert_batch(ref, want_bgr, outside, "the remapper that never left three channels")
        for step, n in enumerate((3, 1, 3, 1)):
            r.set_channels(n)
            got = r.remap(gray if n == 1 else bgr)
            assert r.last_path() == ffi.PATH_UNITS, "step %d" % step
            assert_batch(got, want_gray if n == 1 else want_bgr, outside, "step %d, %d channels" % (step, n))
            if n == 3:
                assert np.array_equal(got, ref), "step %d" % step


# ---------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------
def refused(ffi, status):
    msg = ffi.lib().bevw_last_error().decode()
    assert status == -1 and "channel" in msg, (status, msg)


def test_refusals(ffi):
    from cameracalibration_amd.Tools import undistort as U

    L = ffi.lib()
    size = CM.SMALL
    sw, sh, dw, dh = size
    maps = CM.family("transpose", *size)
    with Remapper(ffi, maps, size, channels=3) as r:
        for n in (0, 2, 4, -1):
            refused(ffi, L.bevw_remapper_set_channels(r.r, n))
        assert L.bevw_remapper_channels(r.r) == 3
        # one channel on a remapper that is not BGR in and out with dense rows
        for fmt in (ffi.INPUT_NV12, ffi.INPUT_YUYV, ffi.INPUT_UYVY):
            ffi.check(L.bevw_remapper_set_input_format(r.r, fmt))
            refused(ffi, L.bevw_remapper_set_channels(r.r, 1))
        ffi.check(L.bevw_remapper_set_input_format(r.r, ffi.INPUT_NV12))
        ffi.check(L.bevw_remapper_set_input_pitch(r.r, sw + 4))
        refused(ffi, L.bevw_remapper_set_channels(r.r, 1))
        ffi.check(L.bevw_remapper_set_input_format(r.r, ffi.INPUT_BGR))
        ffi.check(L.bevw_remapper_set_output_format(r.r, ffi.OUTPUT_NV12))
        refused(ffi, L.bevw_remapper_set_channels(r.r, 1))
        ffi.check(L.bevw_remapper_set_output_format(r.r, ffi.OUTPUT_BGR))
        assert L.bevw_remapper_channels(r.r) == 3
        # ... and the other way round
        r.set_channels(1)
        for fmt in (ffi.INPUT_NV12, ffi.INPUT_YUYV, ffi.INPUT_UYVY):
            refused(ffi, L.bevw_remapper_set_input_format(r.r, fmt))
        refused(ffi, L.bevw_remapper_set_output_format(r.r, ffi.OUTPUT_NV12))
        refused(ffi, L.bevw_remapper_set_input_pitch(r.r, sw + 4))
        d = ffi.DeviceBuffer(dw * dh + sw * sh * 2)
        try:
            table = np.array([[d.ptr, d.ptr + sw * sh]], np.uint64)
            refused(ffi, L.bevw_remap_surfaces_device(r.r, ffi.ptr(table), 1, d.ptr))
            refused(ffi, L.bevw_remap_surface_table_device(r.r, d.ptr, 1, d.ptr))
        finally:
            d.free()
        # what a one-channel remapper already is stays allowed, and it still works
        ffi.check(L.bevw_remapper_set_input_format(r.r, ffi.INPUT_BGR))
        ffi.check(L.bevw_remapper_set_output_format(r.r, ffi.OUTPUT_BGR))
        ffi.check(L.bevw_remapper_set_input_pitch(r.r, 0))
        assert L.bevw_remapper_channels(r.r) == 1
        frames = gray_frames(sw, sh, 1, 995)
        assert np.array_equal(r.remap(frames)[0], CM.numpy_remap(replicate(frames)[0], *maps)[..., 0])
    # an odd source size: the channel count is named before NV12's own size rule; an unknown format keeps its own message
    odd = (255, 191, 160, 120)
    with Remapper(ffi, CM.family("transpose", *odd), odd, channels=1) as r:
        for fmt in (ffi.INPUT_NV12, ffi.INPUT_YUYV, ffi.INPUT_UYVY):
            refused(ffi, L.bevw_remapper_set_input_format(r.r, fmt))
        assert L.bevw_remapper_set_input_format(r.r, 2) == -1 and b"unknown input format" in L.bevw_last_error()
    # Python
    K, D = W.undistort_calibration()
    und = U.Undistorter(K, D, 64, 48, channels=1)
    try:
        assert und.out_image_bytes == und.out_w * und.out_h
        with pytest.raises(Exception, match=r"\[B, height, width\]"):
            und(np.zeros((2, 48, 64, 3), np.uint8))
        with pytest.raises(Exception, match=r"\[B, height, width\]"):
            und(np.zeros((48, 64), np.uint16))
    finally:
        und.close()
    with pytest.raises(Exception, match="channels should be 1/3"):
        U.Undistorter(K, D, 64, 48, channels=2)
    with pytest.raises(Exception, match="channels=1"):
        U.Undistorter(K, D, 64, 48, channels=1, input_format="nv12")


# ---------------------------------------------------------------------------------------------------------------
# 9. InCalibrator.undistort on a [FH, FW] image
# ---------------------------------------------------------------------------------------------------------------
def test_incalibrator_undistort_gray(ffi, oracle):
    from cameracalibration_amd.IntrinsicCalibration.intrinsicCalib import InCalibrator

    a = InCalibrator.get_args()
    saved = (a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE)
    w, h = 320, 256
    try:
        a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE = w, h, FOCAL_SCALE, 1
        K, D = W.undistort_calibration()
        K = np.diag([w / 1280.0, w / 1280.0, 1.0]) @ np.asarray(K, np.float64).reshape(3, 3)
        cal = InCalibrator("fisheye")
        data = cal.set_calibration(K, D)
        Kd = oracle.camera_mat_dst(K, w, h, FOCAL_SCALE, 1)
        m1, m2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, (w, h))
        assert np.array_equal(data.map1, m1) and np.array_equal(data.map2, m2)
        outside = outside_of(m1, w, h)
        assert outside.any()
        bgr = np.random.default_rng(996).integers(0, 256, (h, w, 3), dtype=np.uint8)
        gray = gray_frames(w, h, 1, 997)[0]
        before = cal.undistort(bgr)
        assert_same(before, oracle.remap(bgr, m1, m2), outside, "three channels")
        got = cal.undistort(gray)
        assert got.shape == (h, w)
        assert_same(got, oracle.remap(gray, m1, m2), outside, "one channel")
        assert np.array_equal(cal.undistort(bgr), before)            # a following three-channel call is unchanged
        assert np.array_equal(cal.undistort(gray), got)
        with pytest.raises(Exception, match="FRAME"):
            cal.undistort(np.zeros((h, w + 4), np.uint8))
        cal.camera._release()
        assert cal.camera._remapper is None and cal.camera._remapper_gray is None
    finally:
        a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE = saved
