"""The one-channel stitch on the GPU: BevGenerator(channels=1) / bevw_set_channels against the specification of tests/_gray_stitch.py
(the reference's __call__ with its cv2 calls made on (H, W) arrays, over the committed oracle) at tolerance 0.  The pixels no camera covers
are asserted first (0, or the car), and every case asserts the path that served it (bevw_last_path).  The small rig (320 x 256 frames to a
248 x 250 BEV, car 62 x 100) unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import _gray_stitch as GS
from tests import _harness as H
from tests import _rigs as R
from tests import _shard_cases as SC
from tests._harness import ffi, SB  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = H.SMALL_CFG
NBIG = 33


class Small:
    """The oracle's side of the small rig, computed on first use and left unchanged: generators per blend, NBIG frame sets, a car,
    the specification per (blend, car)."""

    def __init__(self):
        O.build()
        rng = np.random.default_rng(1702)
        self.frames, self.car, self.refs, self.cache = GS.gray_frames(rng, CFG, NBIG), GS.gray_car(rng, CFG), {}, {}

    def ref(self, blend):
        if blend not in self.refs:
            self.refs[blend] = O.RefBevGenerator(H.small_rig(), CFG, blend=blend)
        return self.refs[blend]

    def none(self, blend):
        return H.uncovered(self.ref(blend))

    def want(self, blend, with_car, n):
        key = (blend, with_car)
        have = self.cache.get(key)
        if have is None or have.shape[0] < n:
            self.cache[key] = have = GS.spec_batch(O, self.ref(blend), self.frames[:n], self.car if with_car else None)
        return have[:n]


@pytest.fixture(scope="module")
def small():
    return Small()


def gen(SB, rig=None, cfg=CFG, **kw):
    return H.generator(SB, H.small_rig() if rig is None else rig, cfg, channels=1, **kw)


def dense(img, bw):
    return np.ascontiguousarray(img[..., :bw])


# ---- 1. modes and schedules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_car", [True, False], ids=["car", "nocar"])
@pytest.mark.parametrize("sched", ["auto", "per_pixel"])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_modes_and_schedules(ffi, SB, small, blend, sched, with_car):
    bev = gen(SB, blend=blend, schedule=ffi.SCHED_PER_PIXEL if sched == "per_pixel" else ffi.SCHED_AUTO)
    assert bev.channels == 1 and ffi.lib().bevw_channels(bev._engine.h) == 1
    car = small.car if with_car else None
    got, path = GS.run_device(ffi, bev, small.frames[:5], car)
    assert path == (ffi.PATH_PER_PIXEL if sched == "per_pixel" else ffi.PATH_UNITS)
    assert bev.out_pitch == (CFG["BEV_WIDTH"] if sched == "per_pixel" else 256) and bev.out_image_bytes == bev.out_pitch * CFG["BEV_HEIGHT"]
    assert bev.in_set_bytes == 4 * CFG["FRAME_WIDTH"] * CFG["FRAME_HEIGHT"]
    GS.assert_images(dense(got, CFG["BEV_WIDTH"]), small.want(blend, with_car, 5), small.none(blend), car, "blend %d %s car %d" % (blend, sched, with_car))


# ---- 2. engine against engine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_gray_is_channel_0_of_the_bgr_generator(ffi, SB, small, blend):
    frames = small.frames[:3]
    bgr = H.generator(SB, H.small_rig(), CFG, blend=blend)
    want = bgr.batch(np.repeat(frames[..., None], 3, axis=-1), np.repeat(small.car[..., None], 3, axis=-1))
    assert bgr.last_path() == ffi.PATH_UNITS
    bev = gen(SB, blend=blend)
    got = bev.batch(frames, small.car)
    assert bev.last_path() == ffi.PATH_UNITS
    for k in range(3):
        H.assert_equal(got, np.ascontiguousarray(want[..., k]), "blend %d, channel %d of the BGR generator" % (blend, k))


# ---- 3. saturation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend,white_car", [(False, False), (True, False), (False, True), (True, True)], ids=["direct", "blend", "direct_car", "blend_car"])
def test_saturation_on_white_frames(ffi, SB, small, blend, white_car):
    frames = np.full((2, 4, CFG["FRAME_HEIGHT"], CFG["FRAME_WIDTH"]), 255, np.uint8)
    car = np.full((CFG["BEV_HEIGHT"], CFG["BEV_WIDTH"]), 255, np.uint8) if white_car else None
    ref = small.ref(blend)
    want = GS.spec_batch(O, ref, frames, car)
    two = GS.contributors(ref) == 2
    if not blend:   # 255 + 255 on a seam: 255, where a wrapping add reads 254
        assert two.sum() > 100 and (want[0][two] == 255).sum() > 100 and not (want[0][two] == 254).any()
    bev = gen(SB, blend=blend)
    got, path = GS.run_device(ffi, bev, frames, car)
    assert path == ffi.PATH_UNITS
    GS.assert_images(dense(got, CFG["BEV_WIDTH"]), want, small.none(blend), car, "white frames, blend %d, white car %d" % (blend, white_car))


# ---- 4. rows ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch,px", [("dense", 248), ("aligned", 256), (252, 252)], ids=["dense", "aligned", "252"])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_output_pitch(ffi, SB, small, blend, pitch, px):
    bev = gen(SB, blend=blend, output_pitch=pitch)
    assert bev.out_pitch == px and bev.out_image_bytes == px * CFG["BEV_HEIGHT"]
    got, path = GS.run_device(ffi, bev, small.frames[:3], small.car)   # exactly the batch's bytes between guards
    assert path == ffi.PATH_UNITS and got.shape == (3, CFG["BEV_HEIGHT"], px)
    GS.assert_images(dense(got, 248), small.want(blend, True, 3), small.none(blend), small.car, "pitch %s, blend %d" % (pitch, blend))
    host = bev.batch(small.frames[:3], small.car)                      # the host entry compacts the rows
    GS.assert_images(host, small.want(blend, True, 3), small.none(blend), small.car, "pitch %s, blend %d, host entry" % (pitch, blend))


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_bev_width_250(ffi, SB, small, blend):
    """bw % 4 == 2: dense rows hold no whole quads (per pixel: one channel has no padded scratch); rows of 256 go to the units, the car
    copied to the images' pitch.  The same images."""
    cfg = dict(CFG, BEV_WIDTH=250)
    ref = O.RefBevGenerator(H.small_rig(), cfg, blend=blend)
    rng = np.random.default_rng(5)
    frames, car = GS.gray_frames(rng, cfg, 3), GS.gray_car(rng, cfg)
    want, none = GS.spec_batch(O, ref, frames, car), H.uncovered(ref)
    for pitch, px, path in (("dense", 250, ffi.PATH_PER_PIXEL), ("aligned", 256, ffi.PATH_UNITS)):
        bev = gen(SB, cfg=cfg, blend=blend, output_pitch=pitch)
        got, served = GS.run_device(ffi, bev, frames, car)
        assert bev.out_pitch == px and served == path, (pitch, served)
        GS.assert_images(dense(got, 250), want, none, car, "BEV_WIDTH 250, %s rows, blend %d" % (pitch, blend))
        got, served = GS.run_device(ffi, bev, frames, None)
        assert served == path
        GS.assert_images(dense(got, 250), GS.spec_batch(O, ref, frames, None), none, None, "BEV_WIDTH 250, %s rows, blend %d, no car" % (pitch, blend))


# ---- 5. batch loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_batches_17_and_33_on_one_handle(ffi, SB, small, blend):
    bev = gen(SB, blend=blend)
    for B in (17, 33):   # chunks of 2 and of 8 frames: the chunk tail re-writes its last frame
        got, path = GS.run_device(ffi, bev, small.frames[:B], small.car)
        assert path == ffi.PATH_UNITS
        GS.assert_images(dense(got, 248), small.want(blend, True, B), small.none(blend), small.car, "batch %d, blend %d" % (B, blend))


# ---- 6. frame width ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_frame_width_322(ffi, SB, small, blend):
    cfg = dict(CFG, FRAME_WIDTH=322, FRAME_HEIGHT=258)
    ref = O.RefBevGenerator(H.small_rig(), cfg, blend=blend)
    rng = np.random.default_rng(6)
    frames, car = GS.gray_frames(rng, cfg, 3), GS.gray_car(rng, cfg)
    bev = gen(SB, cfg=cfg, blend=blend, output_pitch="dense")
    got, path = GS.run_device(ffi, bev, frames, car)
    assert path == ffi.PATH_PER_PIXEL   # FW % 4 != 0: no unit list
    GS.assert_images(got, GS.spec_batch(O, ref, frames, car), H.uncovered(ref), car, "322 x 258 frames, blend %d" % blend)


# ---- 7. addresses ------------------------------------------------------------------------------------------------------------------------------
def test_odd_addresses_run_per_pixel_and_the_next_step_is_back_on_the_units(ffi, SB, small):
    bev = gen(SB, blend=True, output_pitch="dense")
    want, none = small.want(True, True, 3), small.none(True)
    for kw in (dict(off_frames=1), dict(off_out=2), dict(off_car=1)):
        got, path = GS.run_device(ffi, bev, small.frames[:3], small.car, **kw)
        assert path == ffi.PATH_PER_PIXEL, kw
        GS.assert_images(got, want, none, small.car, "dense handle, %s" % kw)
        got, path = GS.run_device(ffi, bev, small.frames[:3], small.car)
        assert path == ffi.PATH_UNITS, "the next aligned step"
        GS.assert_images(got, want, none, small.car, "dense handle, aligned after %s" % kw)


def test_a_pitched_handle_refuses_a_misaligned_step_and_writes_nothing(ffi, SB, small):
    bev = gen(SB, output_pitch="aligned")
    got, path = GS.run_device(ffi, bev, small.frames[:2], small.car)
    assert path == ffi.PATH_UNITS
    need = 2 * bev.out_image_bytes
    d_in, d_out, d_car = ffi.DeviceBuffer(small.frames[:2].nbytes + 8), ffi.DeviceBuffer(need + 64), ffi.DeviceBuffer(small.car.nbytes + 8)
    try:
        d_in.upload(small.frames[:2], 1)
        d_car.upload(small.car, 1)
        for frames_p, car_p, out_p in ((d_in.ptr + 1, d_car.ptr, d_out.ptr), (d_in.ptr, d_car.ptr + 1, d_out.ptr), (d_in.ptr, d_car.ptr, d_out.ptr + 2)):
            d_out.fill(GS.FILL)
            with pytest.raises(ffi.BevwError, match="4-byte aligned"):
                bev.run_device(frames_p, 2, car_p, out_p, out_bytes=need)
            bev.sync()
            assert (d_out.download((need + 64,)) == GS.FILL).all(), "a refused step wrote something"
            assert bev.last_path() == ffi.PATH_UNITS   # a refused step leaves it unchanged
    finally:
        for d in (d_in, d_out, d_car):
            d.free()


# ---- 8. geometries -----------------------------------------------------------------------------------------------------------------------------
def _case(SB, ffi, rig, cfg, blend, seed):
    ref = O.RefBevGenerator(rig, cfg, blend=blend)
    rng = np.random.default_rng(seed)
    frames = GS.gray_frames(rng, cfg, 2)
    car = GS.gray_car(rng, cfg) if cfg["CAR_WIDTH"] and cfg["CAR_HEIGHT"] else None
    bev = gen(SB, rig=rig, cfg=cfg, blend=blend)
    got, path = GS.run_device(ffi, bev, frames, car)
    return bev, ref, frames, car, dense(got, cfg["BEV_WIDTH"]), path


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_a_bev_without_a_car_runs_per_pixel(ffi, SB, blend):
    cfg = SC.geo_cfg((252, 180, 0, 0))
    bev, ref, frames, car, got, path = _case(SB, ffi, H.small_rig(), cfg, blend, 81)
    assert GS.contributors(ref).max() > 2 and not bev.plan_info()["plan_usable"] and path == ffi.PATH_PER_PIXEL
    GS.assert_images(got, GS.spec_batch(O, ref, frames, car), H.uncovered(ref), car, "no car, blend %d" % blend)


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_a_car_as_wide_as_the_bev(ffi, SB, blend):
    cfg = SC.geo_cfg((260, 250, 260, 100))
    bev, ref, frames, car, got, path = _case(SB, ffi, H.small_rig(), cfg, blend, 82)
    if not blend:
        assert any(not np.asarray(m).any() for m in ref.masks), "a direct mask is empty"
    assert path == ffi.PATH_UNITS
    GS.assert_images(got, GS.spec_batch(O, ref, frames, car), H.uncovered(ref), car, "car as wide as the BEV, blend %d" % blend)


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
@pytest.mark.parametrize("name", ["roll90", "mirrored", "same4", "barrel_strong", "pincushion"])
def test_rig_families(ffi, SB, name, blend):
    rig, cfg = R.family(name)
    bev, ref, frames, car, got, path = _case(SB, ffi, rig, cfg, blend, 83)
    assert path == ffi.PATH_UNITS
    if name in R.BORDER:
        assert bev.plan_info()["tiles_border"] > 0, "the per-tap kernel serves border tiles of this family"
    GS.assert_images(got, GS.spec_batch(O, ref, frames, car), H.uncovered(ref), car, "%s, blend %d" % (name, blend))


# ---- 9. setter walk ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_setter_walk_on_one_built_handle(ffi, SB, small, blend):
    L = ffi.lib()
    frames, car = small.frames[:3], small.car
    bgr_frames, bgr_car = np.repeat(frames[..., None], 3, axis=-1), np.repeat(car[..., None], 3, axis=-1)
    bgr_frames[..., 1] //= 2   # (three different channels: a BGR step is not three grey ones)
    fresh = H.generator(SB, H.small_rig(), CFG, blend=blend)
    want_bgr = fresh.batch(bgr_frames, bgr_car)
    bev = H.generator(SB, H.small_rig(), CFG, blend=blend)
    for n in (3, 1, 3, 1):
        ffi.check(L.bevw_set_channels(bev._engine.h, n))
        assert L.bevw_channels(bev._engine.h) == n
        bev.channels = n
        if n == 3:
            H.assert_equal(bev.batch(bgr_frames, bgr_car), want_bgr, "BGR step of the walk, blend %d" % blend)
        else:
            GS.assert_images(bev.batch(frames, car), small.want(blend, True, 3), small.none(blend), car, "grey step of the walk, blend %d" % blend)
        assert bev.last_path() == ffi.PATH_UNITS


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------------
def _refused(ffi, status):
    err = ffi.lib().bevw_last_error()
    assert status == -1 and (b"1 channel" in err or b"channel count 1" in err), (status, err)


def test_refusals_in_both_orders(ffi, SB, small):
    L = ffi.lib()
    fw, fh, bw, bh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"], CFG["BEV_WIDTH"], CFG["BEV_HEIGHT"]
    cams = np.array([0, 1], np.int32)

    def fresh(first=None):
        h = H.raw_handle(ffi, fw, fh, bw, bh)
        if first:
            ffi.check(first(h))
        return h

    one = lambda h: L.bevw_set_channels(h, 1)
    setters = [lambda h: L.bevw_set_input_format(h, ffi.INPUT_NV12), lambda h: L.bevw_set_input_format(h, ffi.INPUT_YUYV),
               lambda h: L.bevw_set_input_format(h, ffi.INPUT_UYVY), lambda h: L.bevw_set_output_format(h, ffi.OUTPUT_NV12),
               lambda h: L.bevw_set_projection(h, ffi.PROJ_ANALYTIC), lambda h: L.bevw_set_projection(h, ffi.PROJ_ANALYTIC_F32),
               lambda h: L.bevw_set_camera_shard(h, ffi.ptr(cams), 2)]
    for other in setters:
        for first, second in ((other, one), (one, other)):
            h = fresh(first)
            try:
                _refused(ffi, second(h))
                assert L.bevw_channels(h) == (1 if first is one else 3)
            finally:
                L.bevw_destroy(h)
    # an input pitch exists with NV12 input alone, which refuses the channel count already; the other order:
    h = fresh(one)
    try:
        _refused(ffi, L.bevw_set_input_pitch(h, fw + 4))
        assert L.bevw_set_channels(h, 2) == -1 and L.bevw_set_channels(h, 3) == 0 and L.bevw_channels(h) == 3
    finally:
        L.bevw_destroy(h)
    h = fresh(lambda h: L.bevw_set_input_format(h, ffi.INPUT_NV12))
    try:
        ffi.check(L.bevw_set_input_pitch(h, fw + 4))
        _refused(ffi, one(h))
    finally:
        L.bevw_destroy(h)
    # a handle created with balance = 1
    cfg = ffi.bevw_config(fw, fh, bw, bh, 62, 100, 1.0, 2.0, 1, 1, 0, 0)
    h = C.c_void_p()
    ffi.check(L.bevw_create(C.byref(cfg), C.byref(h)))
    try:
        _refused(ffi, one(h))
        assert b"balance" in L.bevw_last_error()
    finally:
        L.bevw_destroy(h)
    # the surface entry points and bevw_combine_device on a built one-channel handle
    bev = gen(SB)
    d = ffi.DeviceBuffer(bev.out_image_bytes)
    try:
        table = np.full((1, 4, 2), d.ptr, np.uint64)
        box = np.array([0, 0, bw, bh], np.int32)
        parts = (C.c_void_p * 1)(d.ptr)
        _refused(ffi, L.bevw_run_surfaces_device(bev._engine.h, ffi.ptr(table), 1, None, d.ptr))
        _refused(ffi, L.bevw_run_surface_table_device(bev._engine.h, d.ptr, 1, None, d.ptr))
        _refused(ffi, L.bevw_combine_device(bev._engine.h, parts, ffi.ptr(box), 1, 1, None, d.ptr))
        with pytest.raises(Exception, match="channels=3"):
            bev.jpeg([(b"", b"", b"", b"")])
        with pytest.raises(Exception, match="channels=3"):
            next(iter(bev.jpeg_stream([[(b"", b"", b"", b"")]])))
    finally:
        d.free()


# ---- 11. host entry points ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_host_entry_points(ffi, SB, small, blend):
    bev = gen(SB, blend=blend)
    want, none = small.want(blend, True, 4), small.none(blend)
    got = bev(*small.frames[0], small.car)
    assert got.shape == (CFG["BEV_HEIGHT"], CFG["BEV_WIDTH"]) and bev.last_path() == ffi.PATH_UNITS
    GS.assert_images(got[None], want[:1], none, small.car, "__call__, blend %d" % blend)
    GS.assert_images(bev(*small.frames[1])[None], small.want(blend, False, 2)[1:2], none, None, "__call__ without a car, blend %d" % blend)
    got = bev.batch(small.frames[:4], small.car)
    assert bev.last_path() == ffi.PATH_UNITS
    GS.assert_images(got, want, none, small.car, "batch, blend %d" % blend)
    for bad in (small.frames[0][0][..., None], np.repeat(small.frames[0][0][..., None], 3, -1), small.frames[0][0].astype(np.uint16)):
        with pytest.raises(Exception, match="channels=1"):
            bev(bad, bad, bad, bad)
    with pytest.raises(Exception, match="channels=1"):
        bev(*small.frames[0], np.repeat(small.car[..., None], 3, -1))
