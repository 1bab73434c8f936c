"""GPU leg of the calibration-side warps: the catalogue of tests/_calib_warps.py through the C ABI and the Python mirrors, in-process, at
tolerance 0 against the oracle (tests/test_calib_warps_host.py holds the oracle against its NumPy twins and against exact arithmetic).

Every call runs a batch of CW.BATCH distinct images over a 0x5a fill with a guard image behind the last one.  Reading perspective_coord,
remap_u8c3_px, warp_f32_px and the two map kernels, every tap index is range-checked after the clamp: no family here can address outside
the source."""
import ctypes as C

import numpy as np
import pytest

from tests import _calib_warps as CW
from tests._harness import assert_equal, ffi  # noqa: F401

pytestmark = pytest.mark.gpu
FILL = 0x5A
E_INVALID = -1


def guarded(n, shape):
    """n images of `shape` and a guard image behind them, all FILL"""
    return np.full((n + 1,) + tuple(shape), FILL, np.uint8)


def assert_guard(buf, what):
    assert (buf[-1] == FILL).all(), "%s: %d bytes behind the last image were written" % (what, int((buf[-1] != FILL).sum()))


def warp(ffi, imgs, H, dsize, what):
    """bevw_warp_perspective_u8c3 on a batch [n, sh, sw, 3] -> [n, dh, dw, 3]"""
    n, sh, sw = imgs.shape[:3]
    buf = guarded(n, (dsize[1], dsize[0], 3))
    ffi.check(ffi.lib().bevw_warp_perspective_u8c3(0, ffi.ptr(np.ascontiguousarray(imgs)), sw, sh, ffi.ptr(ffi.f64(H, 9)), dsize[0], dsize[1], n,
                                                   ffi.ptr(buf)))
    assert_guard(buf, what)
    return buf[:n]


def check_warp(ffi, oracle, name, src, dsize, imgs):
    H = CW.homography(name, src, dsize)
    what = "%s, source %s -> %s" % (name, src, dsize)
    got = warp(ffi, imgs, H, dsize, what)
    for b in range(imgs.shape[0]):
        assert_equal(got[b], oracle.warp_perspective(imgs[b], H, dsize), "%s, image %d" % (what, b))
    return got


@pytest.mark.parametrize("name", CW.FAMILIES)
def test_classic_warp(ffi, oracle, name):
    """k_warp_perspective, classic: every destination size (block widths 146, 1024, 257, 68, 64 and 1) on the 96 x 64 source, and the odd,
    one-texel, one-column and two-row sources on the families that still show them"""
    assert ffi.lib().bevw_get_compat(ffi.COMPAT_WARP) == 0
    imgs = CW.images(CW.SRC)
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2]) and imgs.shape[0] == CW.BATCH == 3
    for dsize in CW.DSIZES:
        got = check_warp(ffi, oracle, name, CW.SRC, dsize, imgs)
        if name == "singular":   # every pixel is src[0, 0]
            assert all((got[b] == imgs[b][0, 0]).all() for b in range(3))
        if name == "far_translate":
            assert not got.any()
    if name in CW.ON_SOURCES:
        for src in CW.SOURCES:
            for dsize in CW.DSIZES:
                got = check_warp(ffi, oracle, name, src, dsize, CW.images(src))
                assert got.any(), (name, src, dsize)


@pytest.mark.parametrize("name", CW.FAMILIES)
def test_excalibrator_warp_catalogue(ffi, oracle, name):
    """ExCalibrator.warp: dst_img once as an array, once as a (height, width) pair; the source a non-contiguous view"""
    from cameracalibration_amd.ExtrinsicCalibration import ExCalibrator

    sw, sh = CW.SRC
    big = np.random.default_rng(17).integers(0, 256, (sh * 2, sw + 9, 3), dtype=np.uint8)
    view = big[1::2, 4:4 + sw]
    assert not view.flags["C_CONTIGUOUS"] and view.shape == (sh, sw, 3)
    dsize = (131, 67)
    H = CW.homography(name, CW.SRC, dsize)
    want = oracle.warp_perspective(np.ascontiguousarray(view), H, dsize)
    ex = ExCalibrator()
    ex.set_homography(H, view, np.zeros((dsize[1], dsize[0], 3), np.uint8))
    assert_equal(ex.warp(), want, name + ", dst_img an array")
    ex.set_homography(H, view, (dsize[1], dsize[0]))
    assert_equal(ex.warp(), want, name + ", dst_img a (height, width) pair")


@pytest.mark.parametrize("name", CW.F32_FAMILIES)
def test_float32_family(ffi, oracle, name):
    """k_warp_perspective through all 32 members of the float32 family (BEVW_COMPAT_WARP / VARIANT_WARP)"""
    L = ffi.lib()
    imgs = CW.images(CW.SRC)
    assert len(CW.F32_MODES) == 32
    results = {}
    try:
        for dsize in CW.EXACT_DSIZES:
            H = CW.homography(name, CW.SRC, dsize)
            for mode in CW.F32_MODES:
                ffi.check(L.bevw_set_compat(ffi.COMPAT_WARP, mode))
                oracle.set_variant(oracle.VARIANT_WARP, mode)
                assert L.bevw_get_compat(ffi.COMPAT_WARP) == mode
                results[dsize, mode] = check_warp(ffi, oracle, name, CW.SRC, dsize, imgs).copy()
    finally:
        L.bevw_set_compat(ffi.COMPAT_WARP, 0)
        oracle.set_variant(oracle.VARIANT_WARP, 0)
    assert L.bevw_get_compat(ffi.COMPAT_WARP) == 0 and oracle.get_variant(oracle.VARIANT_WARP) == 0
    if name != "far_translate":   # the members are not one kernel under 32 names: some pair of them differs, and the image is shown
        assert any(not np.array_equal(results[d, 1], results[d, m]) for d in CW.EXACT_DSIZES for m in CW.F32_MODES)
        assert all(results[d, 1].any() for d in CW.EXACT_DSIZES)
    else:
        assert not any(r.any() for r in results.values())


# ---------------------------------------------------------------------------------------------------------------
# the map builders
# ---------------------------------------------------------------------------------------------------------------
def check_remapper(ffi, oracle, r, want_maps, what):
    L = ffi.lib()
    try:
        m1, m2 = want_maps
        dims = np.zeros(4, np.int32)
        ffi.check(L.bevw_remapper_dims(r, ffi.ptr(dims)))
        assert dims.tolist() == [CW.FRAME[0], CW.FRAME[1], m2.shape[1], m2.shape[0]], what
        g1, g2 = np.full(m1.shape, 0x5a5a, np.int16), np.full(m2.shape, 0x5a5a, np.uint16)
        ffi.check(L.bevw_remapper_get_maps(r, ffi.ptr(g1), ffi.ptr(g2)))
        assert_equal(g1, m1, what + ", map1")
        assert_equal(g2, m2, what + ", map2")
        frames = CW.frames(2)
        buf = guarded(2, m2.shape + (3,))
        ffi.check(L.bevw_remap(r, ffi.ptr(frames), 2, ffi.ptr(buf)))
        assert_guard(buf, what)
        for b in range(2):
            assert_equal(buf[b], oracle.remap(frames[b], m1, m2), "%s, frame %d" % (what, b))
    finally:
        L.bevw_remapper_destroy(r)


@pytest.mark.parametrize("name", list(CW.PINHOLE_SETS))
def test_pinhole_remapper(ffi, oracle, name):
    """k_pinhole_map through bevw_pinhole_remapper_create: far-out entries wrap in the (int16) store, as the oracle's do"""
    D, fs, ss, oh, ov = CW.PINHOLE_SETS[name]
    Kd = oracle.camera_mat_dst(CW.PINHOLE_K, CW.FRAME[0], CW.FRAME[1], fs, ss, oh, ov)
    want = oracle.init_undistort_rectify_map(CW.PINHOLE_K, D, Kd, CW.map_size(ss))
    r = C.c_void_p()
    d = np.ascontiguousarray(D, np.float64) if len(D) else np.zeros(1)
    ffi.check(ffi.lib().bevw_pinhole_remapper_create(0, CW.FRAME[0], CW.FRAME[1], ffi.ptr(ffi.f64(CW.PINHOLE_K, 9)), ffi.ptr(d), len(D), fs, ss, oh, ov,
                                                     C.byref(r)))
    check_remapper(ffi, oracle, r, want, "pinhole set " + name)


@pytest.mark.parametrize("name", list(CW.FISHEYE_SETS))
def test_fisheye_remapper(ffi, oracle, name):
    """k_fisheye_map through a stand-alone remapper with offsets and scales"""
    k, fs, ss, oh, ov = CW.FISHEYE_SETS[name]
    K, D = CW.fisheye_calibration(k)
    Kd = oracle.camera_mat_dst(K, CW.FRAME[0], CW.FRAME[1], fs, ss, oh, ov)
    want = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, CW.map_size(ss))
    r = C.c_void_p()
    ffi.check(ffi.lib().bevw_fisheye_remapper_create(0, CW.FRAME[0], CW.FRAME[1], ffi.ptr(ffi.f64(K, 9)), ffi.ptr(ffi.f64(D, 4)), fs, ss, oh, ov, C.byref(r)))
    check_remapper(ffi, oracle, r, want, "fisheye set " + name)


def test_incalibrator_normal_four_coefficients(ffi, oracle):
    from cameracalibration_amd.IntrinsicCalibration import InCalibrator

    a = InCalibrator.get_args()
    keep = (a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE)
    D, fs, ss = CW.PINHOLE_SETS["d4"][:3]
    try:
        a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE = CW.FRAME[0], CW.FRAME[1], fs, ss
        cal = InCalibrator("normal")
        data = cal.set_calibration(CW.PINHOLE_K, D)
        Kd = oracle.camera_mat_dst(CW.PINHOLE_K, CW.FRAME[0], CW.FRAME[1], fs, ss)
        m1, m2 = oracle.init_undistort_rectify_map(CW.PINHOLE_K, D, Kd, CW.map_size(ss))
        assert_equal(data.map1, m1, "map1")
        assert_equal(data.map2, m2, "map2")
        frame = CW.frames(1)[0]
        assert_equal(cal.undistort(frame), oracle.remap(frame, m1, m2), "undistort")
    finally:
        a.FRAME_WIDTH, a.FRAME_HEIGHT, a.FOCAL_SCALE, a.SIZE_SCALE = keep


# ---------------------------------------------------------------------------------------------------------------
# resize and translate
# ---------------------------------------------------------------------------------------------------------------
def test_resize_catalogue(ffi, oracle):
    """k_resize_linear: every case of the catalogue, batch 3; bevw_resize_dsize against half-to-even; empty destinations refused"""
    L = ffi.lib()
    ds = np.zeros(2, np.int32)
    for w, h, fx, fy in CW.resize_cases():
        what = "resize %d x %d by (%s, %s)" % (w, h, fx, fy)
        ffi.check(L.bevw_resize_dsize(w, h, fx, fy, ffi.ptr(ds)))
        assert (int(ds[0]), int(ds[1])) == (CW.round_half_even(w * fx), CW.round_half_even(h * fy)), what
        imgs = np.random.default_rng([w, h, 3]).integers(0, 256, (CW.BATCH, h, w, 3), dtype=np.uint8)
        buf = guarded(CW.BATCH, (int(ds[1]), int(ds[0]), 3))
        ffi.check(L.bevw_resize_linear_u8c3(0, ffi.ptr(imgs), w, h, fx, fy, CW.BATCH, ffi.ptr(buf)))
        assert_guard(buf, what)
        for b in range(CW.BATCH):
            assert_equal(buf[b], oracle.resize_linear(imgs[b], fx, fy), "%s, image %d" % (what, b))
    for (w, h, fx, fy), dsize in CW.RESIZE_TIES.items():
        ffi.check(L.bevw_resize_dsize(w, h, fx, fy, ffi.ptr(ds)))
        assert (int(ds[0]), int(ds[1])) == dsize
    one = np.zeros((1, 8, 8, 3), np.uint8)
    for w, h, fx, fy in CW.RESIZE_EMPTY:
        assert L.bevw_resize_dsize(w, h, fx, fy, ffi.ptr(ds)) == E_INVALID
        assert L.bevw_resize_linear_u8c3(0, ffi.ptr(one), w, h, fx, fy, 1, ffi.ptr(one)) == E_INVALID and not one.any()


@pytest.mark.parametrize("size", CW.TRANSLATE_SIZES)
def test_translate_catalogue(ffi, oracle, size):
    """k_translate: shifts through 0, +-1, +-(n - 1), +-n, +-(3 n + 1) and +-2^30 on both axes, batch 3"""
    w, h = size
    imgs = np.random.default_rng([w, h, 4]).integers(1, 256, (CW.BATCH, h, w, 3), dtype=np.uint8)
    for sx, sy in CW.translate_shifts(w, h):
        what = "translate %d x %d by (%d, %d)" % (w, h, sx, sy)
        buf = guarded(CW.BATCH, (h, w, 3))
        ffi.check(ffi.lib().bevw_translate_u8c3(0, ffi.ptr(imgs), w, h, sx, sy, CW.BATCH, ffi.ptr(buf)))
        assert_guard(buf, what)
        for b in range(CW.BATCH):
            assert_equal(buf[b], oracle.translate(imgs[b], sx, sy), "%s, image %d" % (what, b))


def test_scale_and_center_image_mirrors(ffi, oracle):
    """ScaleImage and CenterImage on an image that is not the sample image: 97 x 65, rows that are no dword multiples"""
    from cameracalibration_amd.ExtrinsicCalibration import extrinsicCalib as EC

    img = CW.images((97, 65))[2]
    h, w = img.shape[:2]
    a = EC.ExCalibrator.get_args()
    gx, gy = np.meshgrid(np.arange(a.BORAD_WIDTH), np.arange(a.BORAD_HEIGHT))
    corners = np.stack([10 + gx * 7.1, 5 + gy * 7.1], -1).reshape(-1, 1, 2)
    sc = EC.ScaleImage(corners)
    assert sc.scale_factor > 1
    ref = oracle.resize_linear(img, sc.scale_factor, sc.scale_factor)
    t, l = (ref.shape[0] - h) // 2, (ref.shape[1] - w) // 2
    assert_equal(sc(img), ref[t:t + h, l:l + w], "ScaleImage")
    c = EC.CenterImage().set_center(90, 3)
    assert_equal(c(img), oracle.translate(img, w // 2 - 90, h // 2 - 3), "CenterImage")


# ---------------------------------------------------------------------------------------------------------------
# destinations taller than a grid
# ---------------------------------------------------------------------------------------------------------------
def test_tall_destinations_are_refused(ffi, oracle):
    """65,536 rows do not fit grid.y: bevw_warp_perspective_u8c3 and bevw_translate_u8c3 refuse them with BEVW_E_INVALID on the host, as
    bevw_resize_linear_u8c3 does, and leave the destination alone; 65,535 rows of one pixel run"""
    L = ffi.lib()
    col = np.random.default_rng(6).integers(0, 256, (1, 65536, 1, 3), dtype=np.uint8)
    out = np.full((65536, 1, 3), FILL, np.uint8)
    H = ffi.f64(np.eye(3), 9)
    assert L.bevw_warp_perspective_u8c3(0, ffi.ptr(col), 1, 65536, ffi.ptr(H), 1, 65536, 1, ffi.ptr(out)) == E_INVALID
    assert "65535" in ffi.lib().bevw_last_error().decode()
    assert L.bevw_translate_u8c3(0, ffi.ptr(col), 1, 65536, 0, 1, 1, ffi.ptr(out)) == E_INVALID
    assert "65535" in ffi.lib().bevw_last_error().decode()
    assert L.bevw_resize_linear_u8c3(0, ffi.ptr(col), 1, 65536, 1.0, 1.0, 1, ffi.ptr(out)) == E_INVALID
    assert (out == FILL).all()
    short = np.ascontiguousarray(col[:, :65535])
    ffi.check(L.bevw_warp_perspective_u8c3(0, ffi.ptr(short), 1, 65535, ffi.ptr(H), 1, 65535, 1, ffi.ptr(out)))
    assert_equal(out[:65535], oracle.warp_perspective(short[0], np.eye(3), (1, 65535)), "identity at 65,535 rows")
    # the coordinates saturate at int16: rows up to 32,767 are the source's, every later one shows row 32,767
    assert np.array_equal(out[:32768], short[0, :32768]) and (out[32768:65535] == short[0, 32767]).all()
    assert (out[65535] == FILL).all()
    ffi.check(L.bevw_translate_u8c3(0, ffi.ptr(short), 1, 65535, 0, 1, 1, ffi.ptr(out)))
    assert_equal(out[:65535], oracle.translate(short[0], 0, 1), "translate at 65,535 rows")
    assert (out[65535] == FILL).all()
