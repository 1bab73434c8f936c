"""Nearest-neighbour remapping of one-channel images (bevw_remapper_set_interpolation, Undistorter(channels=1, interpolation='nearest'),
InCalibrator.undistort(mask, interpolation='nearest')) on the GPU: k_units_nn8 / nn16 on the unit schedule, k_tiles_nn8 / nn16 for the
frame-border tiles, k_remap_nn8 / nn16 as the fall-back.

The expected value is always the NumPy statement of cv2's rule (tests/_nearest.py want_nn), compared with tolerance 0 over all pixels, on
label frames (where a blend of two values is the ID of nobody) and on full-range frames.  Pixels whose nearest texel lies outside the frame
are asserted to be 0 on their own first.  Which kernels served a step is asked of the library (bevw_remapper_last_path) and asserted, so
that no case passes through the fall-back unnoticed.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests import _caller_maps as CM
from tests import _gray_maps as GM
from tests import _nearest as NN
from tests._harness import Remapper, ffi, outside_of, run_child  # noqa: F401

pytestmark = pytest.mark.gpu

FOCAL_SCALE = 0.1     # the fisheye view zoomed out until its rim leaves the frame (at the benchmark's 0.5 every pixel samples inside)
CHILD_TIMEOUT = 120   # seconds: a library load and one small remapper take a few seconds
DEPTHS = (8, 16)


# ---------------------------------------------------------------------------------------------------------------
# 1. Undistorter(channels=1, interpolation='nearest')
# ---------------------------------------------------------------------------------------------------------------
def run_undistort(ffi, oracle, w, h, batch, depth, compat, path, seed):
    from cameracalibration_amd.Tools import undistort as U

    cfg = W.CONFIG_UNDISTORT
    K, D = W.undistort_calibration()
    s = w / float(cfg["FRAME_WIDTH"])
    K = np.diag([s, s, 1.0]) @ np.asarray(K, np.float64).reshape(3, 3)   # the calibration scaled to the source size
    L = ffi.lib()
    imgs = NN.label_frames(w, h, batch, seed, depth)
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, compat))
        und = U.Undistorter(K, D, w, h, focalscale=FOCAL_SCALE, sizescale=cfg["SIZE_SCALE"], channels=1, depth=depth, interpolation="nearest")
        try:
            assert und.last_path() == ffi.PATH_NONE and und.interpolation == "nearest"
            assert L.bevw_remapper_interpolation(und._r) == ffi.INTER_NEAREST and L.bevw_remapper_depth(und._r) == depth
            got = und(imgs)
            assert und.last_path() == path, "path %d, expected %d" % (und.last_path(), path)
            assert got.shape == (batch, und.out_h, und.out_w) and got.dtype == imgs.dtype
            one = und(imgs[batch - 1])
            m1, m2 = und.maps()
            Kd = oracle.camera_mat_dst(K, w, h, FOCAL_SCALE, cfg["SIZE_SCALE"])
            o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, (und.out_w, und.out_h))
            assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
            outside = ~NN.inside_nn(o1, o2, w, h)
            assert outside.any(), "the rim is outside the frame"
            NN.assert_batch_nn(got, NN.want_nn(imgs, o1, o2), outside, "%dx%d depth %d compat %d" % (w, h, depth, compat))
            NN.assert_labels(got, depth, "the device result")
            assert np.array_equal(one, got[batch - 1])
            return got
        finally:
            und.close()
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)


@pytest.mark.parametrize("depth", DEPTHS)
def test_undistort_320x256_on_the_units_in_both_compat_modes(ffi, oracle, depth):
    """BEVW_COMPAT_REMAP selects the tie rule of the fixed-point linear path: a nearest remapper has no tie, takes the plan in both modes and
    gives the same bytes."""
    plain = run_undistort(ffi, oracle, 320, 256, 5, depth, 0, ffi.PATH_UNITS, 3000)
    compat = run_undistort(ffi, oracle, 320, 256, 5, depth, 1, ffi.PATH_UNITS, 3000)
    assert np.array_equal(plain, compat)


@pytest.mark.parametrize("depth", DEPTHS)
def test_undistort_66x48_has_no_plan(ffi, oracle, depth):
    run_undistort(ffi, oracle, 66, 48, 5, depth, 0, ffi.PATH_PER_PIXEL, 3010)   # src_w % 4 != 0


# ---------------------------------------------------------------------------------------------------------------
# 2. caller-made maps: every family at every size of the catalogue, batch 2, both depths, label and full-range frames
# ---------------------------------------------------------------------------------------------------------------
UNIT_FAMILIES = ("transpose", "rot180", "magnify16")   # smooth maps inside the frame: the unit schedule owns them whole
STRADDLE_FAMILIES = ("corner", "scatter", "swirl", "strip_w", "strip_h", "strip_w4")   # nearest texel inside, footprint not (tests/test_nearest_host.py)


@pytest.mark.parametrize("name,size", NN.CASES, ids=NN.CASE_IDS)
def test_caller_maps(ffi, name, size):
    sw, sh, dw, dh = size
    m1, m2 = CM.family(name, sw, sh, dw, dh)
    outside = ~NN.inside_nn(m1, m2, sw, sh)
    straddle = ~outside & ~NN.footprint_inside(m1, sw, sh)
    if name in STRADDLE_FAMILIES:
        assert straddle.any()
    seed = 3020 + CM.FAMILIES.index(name)
    with Remapper(ffi, (m1, m2), size, channels=1) as g:
        g.remap(NN.random_frames(sw, sh, 2, seed, 8))
        gray_path = g.last_path()
        NN.set_interpolation(g, True)
        for depth in DEPTHS:
            NN.set_depth(g, depth)
            for make in (NN.label_frames, NN.random_frames):
                frames = make(sw, sh, 2, seed, depth)
                got = NN.remap_nn(g, frames)
                path = g.last_path()
                what = "%s at %s, %d bits, %s" % (name, size, depth, make.__name__)
                NN.assert_batch_nn(got, NN.want_nn(frames, m1, m2), outside, what)
                if make is NN.label_frames:
                    NN.assert_labels(got, depth, what)
                assert path == gray_path and path in (ffi.PATH_UNITS, ffi.PATH_PER_PIXEL), (what, path, gray_path)   # the units exactly where the linear grey remapper runs them
    print("%s %s: nearest path %d, 8-bit linear grey path %d, %d straddling pixels" % (name, size, path, gray_path, int(straddle.sum())))
    if name in UNIT_FAMILIES:
        assert path == ffi.PATH_UNITS


@pytest.mark.parametrize("size", NN.WRAP_SIZES, ids=["wide", "high"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_the_wrap_sources_run_the_per_pixel_kernel(ffi, size, depth):
    """map1 = 32767 with a delta of 1: texel 32768 in an int, -32768 in cv2's short -- 0.  The plan's entries do not carry the wrap, so a
    source beyond 32768 texels never takes the plan in nearest mode (both widths are multiples of 4 and every pointer is aligned)."""
    sw, sh, dw, dh = size
    m1, m2 = NN.wrap_case(size)
    frames = np.maximum(NN.random_frames(sw, sh, 2, 3050, depth), 1)
    want = NN.want_nn(frames, m1, m2)
    assert not np.array_equal(want, NN.want_nn(frames, m1, m2, wrap=False))
    with Remapper(ffi, (m1, m2), size, channels=1) as g:
        NN.set_interpolation(g, True)
        NN.set_depth(g, depth)
        got = NN.remap_nn(g, frames)
        assert g.last_path() == ffi.PATH_PER_PIXEL
    NN.assert_batch_nn(got, want, ~NN.inside_nn(m1, m2, sw, sh), "wrap %s" % (size,))


@pytest.mark.parametrize("depth", DEPTHS)
def test_an_all_ones_frame(ffi, depth):
    size = CM.SMALL
    sw, sh = size[:2]
    m1, m2 = CM.family("swirl", *size)
    frames = np.full((2, sh, sw), (1 << depth) - 1, NN.DTYPE[depth])
    with Remapper(ffi, (m1, m2), size, channels=1) as g:
        NN.set_interpolation(g, True)
        NN.set_depth(g, depth)
        got = NN.remap_nn(g, frames)
        assert g.last_path() == ffi.PATH_UNITS
    want = NN.want_nn(frames, m1, m2)
    assert want.max() == (1 << depth) - 1 and set(np.unique(got).tolist()) <= {0, (1 << depth) - 1}
    NN.assert_batch_nn(got, want, ~NN.inside_nn(m1, m2, sw, sh), "all ones")


# ---------------------------------------------------------------------------------------------------------------
# 3. ragged batch 19 through bevw_remap_device, device buffers of exactly the batch's bytes between guards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "minify8", "edge_shift"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_ragged_batch_19_on_exact_device_buffers(ffi, name, depth):
    """19 frames: chunks of 2 and a last chunk of 1, whose frame ring runs past the chunk's end.  `corner` is the per-pixel family (every
    base tile is a frame-border tile: no unit); `minify8` and `edge_shift` (tests/_gray_maps.py: up to the frame's last texel) run the units."""
    size = CM.SMALL
    sw, sh, dw, dh = size
    m1, m2 = GM.edge_shift(sw, sh, dw, dh) if name == "edge_shift" else CM.family(name, sw, sh, dw, dh)
    frames = NN.random_frames(sw, sh, 19, 3060, depth)
    outside = ~NN.inside_nn(m1, m2, sw, sh)
    d_in, d_out = NN.Guarded(ffi, frames.nbytes).upload(frames), NN.Guarded(ffi, 19 * dw * dh * depth // 8)
    try:
        with Remapper(ffi, (m1, m2), size, channels=1) as g:
            NN.set_depth(g, depth)
            NN.set_interpolation(g, True)
            g.remap_device(d_in.ptr, 19, d_out.ptr)
            path = g.last_path()
        assert path == (ffi.PATH_PER_PIXEL if name == "corner" else ffi.PATH_UNITS)
        NN.assert_batch_nn(d_out.download((19, dh, dw), NN.DTYPE[depth]), NN.want_nn(frames, m1, m2), outside, name)
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 4. what sends a step to the per-pixel kernel; what is refused
# ---------------------------------------------------------------------------------------------------------------
TRIGGERS = [("dst_w_158", 8), ("dst_w_158", 16), ("src_plus_2", 8), ("src_plus_2", 16), ("dst_plus_2", 8), ("dst_plus_2", 16),
            ("src_plus_1", 8), ("dst_plus_1", 8), ("src_plus_3", 8), ("dst_plus_3", 8)]


@pytest.mark.parametrize("trigger,depth", TRIGGERS, ids=["%s-%d" % t for t in TRIGGERS])
def test_fall_back_triggers(ffi, trigger, depth):
    size = (256, 192, 158, 120) if trigger == "dst_w_158" else CM.SMALL
    sw, sh, dw, dh = size
    m1, m2 = CM.family("minify8", sw, sh, dw, dh)
    frames = NN.label_frames(sw, sh, 3, 3070, depth)
    outside = ~NN.inside_nn(m1, m2, sw, sh)
    assert outside.any()
    want = NN.want_nn(frames, m1, m2)
    shift = 0 if trigger == "dst_w_158" else int(trigger[-1])
    out_bytes = 3 * dw * dh * depth // 8
    d_in = NN.Guarded(ffi, frames.nbytes, shift=shift if trigger.startswith("src") else 0).upload(frames)
    d_out = NN.Guarded(ffi, out_bytes, shift=shift if trigger.startswith("dst_plus") else 0)
    d_al, d_al_out = NN.Guarded(ffi, frames.nbytes).upload(frames), NN.Guarded(ffi, out_bytes)
    try:
        with Remapper(ffi, (m1, m2), size, channels=1) as g:
            NN.set_interpolation(g, True)
            NN.set_depth(g, depth)
            if trigger != "dst_w_158":   # the same remapper on aligned pointers runs the units: the trigger is the pointer alone
                g.remap_device(d_al.ptr, 3, d_al_out.ptr)
                assert g.last_path() == ffi.PATH_UNITS
                NN.assert_batch_nn(d_al_out.download((3, dh, dw), NN.DTYPE[depth]), want, outside, "aligned")
            g.remap_device(d_in.ptr, 3, d_out.ptr)
            assert g.last_path() == ffi.PATH_PER_PIXEL
        NN.assert_batch_nn(d_out.download((3, dh, dw), NN.DTYPE[depth]), want, outside, trigger)
    finally:
        for d in (d_in, d_out, d_al, d_al_out):
            d.free()


@pytest.mark.parametrize("which", ["src", "dst"])
def test_an_odd_address_at_16_bits_is_refused_with_nothing_written(ffi, which):
    size = CM.SMALL
    sw, sh, dw, dh = size
    maps = CM.family("minify8", *size)
    frames = NN.random_frames(sw, sh, 2, 3080, 16)
    d_in = NN.Guarded(ffi, frames.nbytes, shift=1 if which == "src" else 0).upload(frames)
    d_out = NN.Guarded(ffi, 2 * dw * dh * 2, shift=1 if which == "dst" else 0)
    try:
        with Remapper(ffi, maps, size, channels=1) as g:
            NN.set_depth(g, 16)
            NN.set_interpolation(g, True)
            L = ffi.lib()
            assert L.bevw_remap_device(g.r, d_in.ptr, 2, d_out.ptr) == -1
            msg = L.bevw_last_error().decode()
            assert "depth 16" in msg and "2-byte aligned" in msg, msg
            ffi.check(L.bevw_remapper_sync(g.r))
            assert g.last_path() == ffi.PATH_NONE
        assert d_out.untouched()
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 5. the setter walk and the refusals
# ---------------------------------------------------------------------------------------------------------------
WALK = (("linear", 8), ("nearest", 8), ("nearest", 16), ("linear", 16), ("nearest", 16), ("linear", 16), ("linear", 8), ("nearest", 8),
        ("linear", 8), ("nearest", 8))


@pytest.mark.parametrize("compat", [0, 1])
def test_setter_walk_linear_nearest_crossed_with_the_depth(ffi, oracle, compat):
    """Every step against the yardstick of its mode.  compat 1: a remapper made under BEVW_COMPAT_REMAP=1 has no plan at creation; its nearest
    (and 16-bit) steps get one, and its 8-bit linear steps before and after stay on the per-pixel kernel with the even-ties bytes."""
    size = CM.SMALL
    sw, sh = size[:2]
    m1, m2 = CM.family("swirl", *size)
    out_lin, out_nn = outside_of(m1, sw, sh), ~NN.inside_nn(m1, m2, sw, sh)
    frames = {d: NN.random_frames(sw, sh, 3, 3090, d) for d in DEPTHS}
    L = ffi.lib()
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, compat))
        oracle.set_variant(oracle.VARIANT_REMAP, compat)
        want = {("nearest", d): NN.want_nn(frames[d], m1, m2) for d in DEPTHS}
        want.update({("linear", d): np.stack([oracle.remap(f, m1, m2) for f in frames[d]]) for d in DEPTHS})
        with Remapper(ffi, (m1, m2), size, channels=1) as r:
            assert L.bevw_remapper_interpolation(r.r) == ffi.INTER_LINEAR
            for step, (mode, depth) in enumerate(WALK):
                if step % 2:   # the two setters in either order
                    NN.set_depth(r, depth)
                    NN.set_interpolation(r, mode == "nearest")
                else:
                    NN.set_interpolation(r, mode == "nearest")
                    NN.set_depth(r, depth)
                got = NN.remap_nn(r, frames[depth])
                NN.assert_batch_nn(got, want[(mode, depth)], out_nn if mode == "nearest" else out_lin, "step %d: %s, %d bits" % (step, mode, depth))
                per_pixel = compat == 1 and (mode, depth) == ("linear", 8)
                assert r.last_path() == (ffi.PATH_PER_PIXEL if per_pixel else ffi.PATH_UNITS), "step %d" % step
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)
        oracle.set_variant(oracle.VARIANT_REMAP, 0)
    assert not np.array_equal(want[("nearest", 8)], want[("linear", 8)]) and not np.array_equal(want[("nearest", 16)], want[("linear", 16)])


def refused(ffi, status):
    msg = ffi.lib().bevw_last_error().decode()
    assert status == -1 and "interpolation" in msg, (status, msg)


def test_refusals_in_both_orders(ffi):
    L = ffi.lib()
    size = CM.SMALL
    sw, sh, dw, dh = size
    m1, m2 = CM.family("transpose", *size)
    with Remapper(ffi, (m1, m2), size, channels=3) as r:
        for v in (2, 3, -1, 7, 16):
            refused(ffi, L.bevw_remapper_set_interpolation(r.r, v))
        refused(ffi, L.bevw_remapper_set_interpolation(r.r, ffi.INTER_NEAREST))   # nearest on three channels
        assert L.bevw_remapper_interpolation(r.r) == ffi.INTER_LINEAR and L.bevw_remapper_channels(r.r) == 3
        ffi.check(L.bevw_remapper_set_interpolation(r.r, ffi.INTER_LINEAR))       # what it already is stays allowed
        r.set_channels(1)
        NN.set_interpolation(r, True)
        for v in (2, -1):
            refused(ffi, L.bevw_remapper_set_interpolation(r.r, v))
        refused(ffi, L.bevw_remapper_set_channels(r.r, 3))                        # ... and three channels on a nearest one
        assert L.bevw_remapper_interpolation(r.r) == ffi.INTER_NEAREST and L.bevw_remapper_channels(r.r) == 1
        ffi.check(L.bevw_remapper_set_channels(r.r, 1))
        # what a one-channel remapper refuses stays refused, by its own message
        for fmt in (ffi.INPUT_NV12, ffi.INPUT_YUYV, ffi.INPUT_UYVY):
            assert L.bevw_remapper_set_input_format(r.r, fmt) == -1 and b"channel" in L.bevw_last_error()
        assert L.bevw_remapper_set_output_format(r.r, ffi.OUTPUT_NV12) == -1 and b"channel" in L.bevw_last_error()
        assert L.bevw_remapper_set_input_pitch(r.r, sw + 4) == -1 and b"channel" in L.bevw_last_error()
        d = ffi.DeviceBuffer(2 * dw * dh + sw * sh * 2)
        try:
            table = np.array([[d.ptr, d.ptr + sw * sh]], np.uint64)
            assert L.bevw_remap_surfaces_device(r.r, ffi.ptr(table), 1, d.ptr) == -1 and b"channel" in L.bevw_last_error()
            assert L.bevw_remap_surface_table_device(r.r, d.ptr, 1, d.ptr) == -1 and b"channel" in L.bevw_last_error()
        finally:
            d.free()
        # ... and it still works
        frames = NN.label_frames(sw, sh, 1, 3095, 8)
        assert np.array_equal(NN.remap_nn(r, frames), NN.want_nn(frames, m1, m2))
        NN.set_interpolation(r, False)
        r.set_channels(3)


# ---------------------------------------------------------------------------------------------------------------
# 6. InCalibrator.undistort(mask, interpolation='nearest')
# ---------------------------------------------------------------------------------------------------------------
def test_incalibrator_undistort_nearest(ffi, oracle):
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
        m1, m2 = data.map1, data.map2
        outside = ~NN.inside_nn(m1, m2, w, h)
        assert outside.any()
        bgr = np.random.default_rng(3096).integers(0, 256, (h, w, 3), dtype=np.uint8)
        gray = NN.random_frames(w, h, 1, 3097, 8)[0]
        before_bgr, before_gray = cal.undistort(bgr), cal.undistort(gray)
        assert np.array_equal(before_bgr, oracle.remap(bgr, m1, m2)) and np.array_equal(before_gray, oracle.remap(gray, m1, m2))
        for depth in DEPTHS:
            mask = NN.label_frames(w, h, 1, 3098, depth)[0]
            got = cal.undistort(mask, interpolation="nearest")
            NN.assert_same_nn(got, NN.want_nn(mask, m1, m2), outside, "%d bits" % depth)
            NN.assert_labels(got, depth, "InCalibrator")
            assert ffi.lib().bevw_remapper_last_path(cal.camera._remapper_nearest[depth]) == ffi.PATH_UNITS
            assert np.array_equal(cal.undistort(mask, "nearest"), got)
        assert np.array_equal(cal.undistort(bgr), before_bgr) and np.array_equal(cal.undistort(gray), before_gray)   # the calls after are unchanged
        with pytest.raises(Exception, match="nearest"):
            cal.undistort(bgr, interpolation="nearest")
        cal.camera._release()
        assert cal.camera._remapper is None and cal.camera._remapper_nearest == {}
    finally:
        a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE = saved


# ---------------------------------------------------------------------------------------------------------------
# 7. the plan's switches: read once per process
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["BEVW_PLAN_UNITS", "BEVW_REMAP_PLAN"])
def test_plan_switches_off(switch):
    run_child("_nearest_worker.py", [switch], {switch: "0"}, timeout=CHILD_TIMEOUT)
