"""NV12 camera frames (bevw_set_input_format, BevGenerator(input_format='nv12'), Undistorter(input_format='nv12')) on the GPU.

The reference result is always the CPU oracle (oracle.RefBevGenerator, oracle.remap) applied to the BGR frames the NumPy specification
(tests/_nv12_spec.py: cv2.cvtColor(f, cv2.COLOR_YUV2BGR_NV12)) makes of the NV12 input, compared with tolerance 0.  Pixels no camera
covers (under the car, the BEV corners) are asserted on their own first: a kernel that lets the conversion of YUV (0, 0, 0) =
(B, G, R) (0, 154, 0) into a tap without a texel fails there by name.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests import _nv12_spec as S
from tests._harness import SAMPLED, SMALL_CFG, SB, assert_same, ffi, generator, random_car, raw_handle, small_rig, uncovered  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# 1. small rig: every mode, both schedules, with and without the car, dense and pitched device images
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ["dense", "auto"])
@pytest.mark.parametrize("with_car", [False, True])
@pytest.mark.parametrize("sched", ["auto", "per_pixel"])
@pytest.mark.parametrize("blend,balance", [(False, False), (True, False), (True, True)])
def test_small_rig_matches_oracle_on_converted_frames(ffi, SB, oracle, blend, balance, sched, with_car, pitch):
    cfg = SMALL_CFG
    rng = np.random.default_rng(1000 + 8 * blend + 4 * balance + 2 * with_car + (pitch == "auto"))
    schedule = ffi.SCHED_PER_PIXEL if sched == "per_pixel" else ffi.SCHED_AUTO
    bev = generator(SB, small_rig(), cfg, blend=blend, balance=balance, schedule=schedule, output_pitch=pitch, input_format="nv12")
    assert lib_format(ffi, bev) == ffi.INPUT_NV12
    if sched == "auto":
        info = bev.plan_info()
        assert info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0   # the unit kernel's NV12 instantiation runs
    ref = oracle.RefBevGenerator(small_rig(), cfg, blend=blend, balance=balance)
    car = random_car(rng, cfg) if with_car else None
    nv = S.random_nv12(rng, (3, 4), cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"])
    none = uncovered(ref)
    assert none.any()
    got = bev.batch(nv, car)
    for b in range(3):
        assert_same(got[b], ref(*S.nv12_to_bgr(nv[b]), car), none, "set %d" % b)
    one = bev(*nv[0], car)
    assert np.array_equal(one, got[0])


def lib_format(ffi, bev):
    return ffi.lib().bevw_input_format(bev._engine.h)


# ---------------------------------------------------------------------------------------------------------------
# 2. BASELINE config 3 / config 4 geometry at batch 256 through run_device, pitched and dense
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_batch(ffi):
    cfg = W.CONFIG_S
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    set_bytes = 4 * fw * fh * 3 // 2
    rng = np.random.default_rng(33)
    host = np.frombuffer(rng.bytes(256 * set_bytes), np.uint8).reshape(256, 4, fh * 3 // 2, fw)
    d = ffi.DeviceBuffer(host.nbytes).upload(host)
    yield host, d
    d.free()


@pytest.mark.parametrize("pitch", ["auto", "dense"])
@pytest.mark.parametrize("blend,balance", [(False, False), (True, True)], ids=["config3", "config4"])
def test_baseline_geometry_batch256_run_device(ffi, SB, oracle, big_batch, blend, balance, pitch):
    cfg = W.CONFIG_S
    host, d_in = big_batch
    bev = generator(SB, W.rig_s(), cfg, blend=blend, balance=balance, output_pitch=pitch, input_format="nv12")
    assert bev.in_set_bytes == host[0].nbytes
    batch = host.shape[0]
    d_out = ffi.DeviceBuffer(batch * bev.out_image_bytes)
    try:
        bev.run_device(d_in.ptr, batch, None, d_out.ptr, out_bytes=d_out.nbytes)
        bev.sync()
        ref = oracle.RefBevGenerator(W.rig_s(), cfg, blend=blend, balance=balance)
        none = uncovered(ref)
        bh, bw = cfg["BEV_HEIGHT"], cfg["BEV_WIDTH"]
        for b in SAMPLED:
            got = d_out.download((bh, bev.out_pitch, 3), offset=b * bev.out_image_bytes)[:, :bw]
            assert_same(got, ref(*S.nv12_to_bgr(host[b])), none, "set %d of 256" % b)
    finally:
        d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# 3. the reference's own four camera images, CONFIG_R, blend + balance, with the car sprite
# ---------------------------------------------------------------------------------------------------------------
def test_reference_images_blend_balance(ffi, SB, oracle, repo_rig):
    cfg = W.CONFIG_R
    frames = repo_rig.frames()
    nv = [S.bgr_to_nv12(f) for f in frames]   # input generation only
    car = SB.padding(repo_rig.image("car"), cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"])
    ref = oracle.RefBevGenerator(W.repo_rig(), cfg, blend=True, balance=True)
    want = ref(*[S.nv12_to_bgr(f) for f in nv], car)
    none = uncovered(ref)
    for sched in (ffi.SCHED_AUTO, ffi.SCHED_PER_PIXEL):
        bev = generator(SB, W.repo_rig(), cfg, blend=True, balance=True, schedule=sched, input_format="nv12")
        assert_same(bev(*nv, car), want, none, "schedule %d" % sched)
        assert_same(bev.batch(np.stack(nv)[None], car)[0], want, none, "batch, schedule %d" % sched)


# ---------------------------------------------------------------------------------------------------------------
# 4. undistort (BASELINE config 2 geometry) at batch 64: the unit plan, and the ties-to-even per-pixel kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties_even", [0, 1])
def test_undistort_batch64(ffi, oracle, ties_even):
    from cameracalibration_amd.Tools import undistort as U

    cfg = W.CONFIG_UNDISTORT
    w, h = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    K, D = W.undistort_calibration()
    L = ffi.lib()
    rng = np.random.default_rng(64 + ties_even)
    nv = S.random_nv12(rng, (64,), w, h)
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_REMAP, ties_even))
        oracle.set_variant(oracle.VARIANT_REMAP, ties_even)
        und = U.Undistorter(K, D, w, h, focalscale=cfg["FOCAL_SCALE"], sizescale=cfg["SIZE_SCALE"], input_format="nv12")
        got = und(nv)
        one = und(nv[5])
        m1, m2 = und.maps()
        Kd = oracle.camera_mat_dst(K, w, h, cfg["FOCAL_SCALE"], cfg["SIZE_SCALE"])
        o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, (und.out_w, und.out_h))
        assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
        outside = (m1[..., 0] < -1) | (m1[..., 0] >= w) | (m1[..., 1] < -1) | (m1[..., 1] >= h)
        for b in range(64):
            assert_same(got[b], oracle.remap(S.nv12_to_bgr(nv[b]), o1, o2), outside, "image %d" % b)
        assert np.array_equal(one, got[5])
        und.close()
    finally:
        L.bevw_set_compat(ffi.COMPAT_REMAP, 0)
        oracle.set_variant(oracle.VARIANT_REMAP, 0)


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(ffi, SB):
    L = ffi.lib()
    E_INVALID = -1
    # analytic projection, in both orders
    with pytest.raises(ffi.BevwError, match="analytic"):
        generator(SB, small_rig(), SMALL_CFG, projection="analytic", input_format="nv12")
    bev = generator(SB, small_rig(), SMALL_CFG, projection="analytic_f32")
    assert L.bevw_set_input_format(bev._engine.h, ffi.INPUT_NV12) == E_INVALID and b"analytic" in L.bevw_last_error()
    # camera-shard handles, in both orders
    h = raw_handle(ffi, 320, 256, 248, 250)
    try:
        ffi.check(L.bevw_set_input_format(h, ffi.INPUT_NV12))
        assert L.bevw_input_format(h) == ffi.INPUT_NV12
        cams = (C.c_int32 * 2)(0, 2)
        assert L.bevw_set_camera_shard(h, cams, 2) == E_INVALID and b"NV12" in L.bevw_last_error()
        assert L.bevw_set_projection(h, ffi.PROJ_ANALYTIC) == E_INVALID and b"NV12" in L.bevw_last_error()
        ffi.check(L.bevw_set_input_format(h, ffi.INPUT_BGR))
        ffi.check(L.bevw_set_camera_shard(h, cams, 2))
        assert L.bevw_set_input_format(h, ffi.INPUT_NV12) == E_INVALID and b"shard" in L.bevw_last_error()
        assert L.bevw_set_input_format(h, 2) == E_INVALID and L.bevw_set_input_format(h, -1) == E_INVALID
    finally:
        L.bevw_destroy(h)
    # odd frame sizes
    for fw, fh in ((321, 256), (320, 257)):
        h = raw_handle(ffi, fw, fh, 248, 250)
        try:
            assert L.bevw_set_input_format(h, ffi.INPUT_NV12) == E_INVALID and b"even" in L.bevw_last_error()
        finally:
            L.bevw_destroy(h)
    rng = np.random.default_rng(5)
    m1 = rng.integers(0, 60, (40, 48, 2)).astype(np.int16)
    m2 = rng.integers(0, 1024, (40, 48)).astype(np.uint16)
    r = C.c_void_p()
    ffi.check(L.bevw_remapper_from_maps(0, 63, 64, ffi.ptr(m1), ffi.ptr(m2), 48, 40, C.byref(r)))
    try:
        assert L.bevw_remapper_set_input_format(r, ffi.INPUT_NV12) == E_INVALID and b"even" in L.bevw_last_error()
    finally:
        L.bevw_remapper_destroy(r)
    # JPEG entry points decode to BGR; shapes
    nvgen = generator(SB, small_rig(), SMALL_CFG, input_format="nv12")
    with pytest.raises(Exception, match="input_format='bgr'"):
        nvgen.jpeg([[b"", b"", b"", b""]])
    with pytest.raises(Exception, match="input_format='bgr'"):
        list(nvgen.jpeg_stream([[[b"", b"", b"", b""]]]))
    fw, fh = SMALL_CFG["FRAME_WIDTH"], SMALL_CFG["FRAME_HEIGHT"]
    bgr = np.zeros((fh, fw, 3), np.uint8)
    with pytest.raises(Exception, match=r"\(384, 320\)"):
        nvgen(bgr, bgr, bgr, bgr)
    with pytest.raises(Exception, match=r"\[B, 4, 384, 320\]"):
        nvgen.batch(np.zeros((1, 4, fh, fw, 3), np.uint8))
    with pytest.raises(Exception, match=r"\(384, 320\)"):
        nvgen(*np.zeros((4, fh * 3 // 2, fw), np.float32))
    with pytest.raises(Exception, match="bgr/nv12"):
        generator(SB, small_rig(), SMALL_CFG, input_format="i420")
    from cameracalibration_amd.Tools import undistort as U

    K, D = W.undistort_calibration()
    und = U.Undistorter(K, D, 64, 48, input_format="nv12")
    with pytest.raises(Exception, match=r"\[B, 72, 64\]"):
        und(np.zeros((2, 48, 64, 3), np.uint8))
    und.close()
