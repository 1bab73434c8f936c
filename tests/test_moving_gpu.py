"""The stitch with a homography per frame set on the GPU: bevw_run_homographies_device / bevw_run_homographies / BevGenerator.batch_homographies
against two yardsticks that do not know the new code, at tolerance 0, the pixels no camera covers first --
  A: per frame set the committed oracle, RefBevGenerator(rig with H_b)(*frames_b, car);
  B: per frame set a fresh BevGenerator(rig with H_b) on the library's existing static path.
Every case asserts the path of the step (bevw_last_path).  The small rig (320 x 256 frames to a 248 x 250 BEV) and batches of 5 unless a case
says otherwise; tests/test_moving_host.py holds the census that says no family below passes emptily."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import _harness as H
from tests import _moving as MV
from tests import _shard_cases as SC
from tests._harness import ffi, SB  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = H.SMALL_CFG
BW = CFG["BEV_WIDTH"]
NBIG = 33
ENTRY = b"bevw_run_homographies_device"


class Small:
    """The oracle's side of the small rig, computed on first use and left unchanged: NBIG frame sets, a car, the rigs of the mixed table
    (frame set b uses rig b % 5) and of the hostile families, yardstick A per (table, blend, car)."""

    def __init__(self):
        O.build()
        rng = np.random.default_rng(1802)
        self.rig = H.small_rig()
        self.frames, self.car, self.cache = MV.frames_for(rng, NBIG), H.random_car(rng, CFG), {}
        self.mixed, self.hostile = MV.mixed_rigs(O, self.rig), MV.hostile_rigs(O, self.rig)
        self.none = H.uncovered(O.RefBevGenerator(self.rig, CFG))

    def rigs(self, kind, n):
        src = self.mixed if kind == "mixed" else self.hostile
        return [src[b % len(src)] for b in range(n)]

    def table(self, kind, n):
        return MV.table(self.rigs(kind, n))

    def want(self, kind, blend, with_car, n):
        key = (kind, blend, with_car)
        have = self.cache.get(key)
        if have is None or have.shape[0] < n:
            src = self.mixed if kind == "mixed" else self.hostile
            refs = [O.RefBevGenerator(r, CFG, blend=blend) for _, r in src]
            car = self.car if with_car else None
            self.cache[key] = have = np.stack([refs[b % len(refs)](*self.frames[b], car) for b in range(n)])
        return have[:n]


@pytest.fixture(scope="module")
def small():
    return Small()


def gen(SB, rig=None, cfg=CFG, **kw):
    return H.generator(SB, H.small_rig() if rig is None else rig, cfg, **kw)


def dense(img, bw=BW):
    return np.ascontiguousarray(img[:, :, :bw])


# ---- 1. modes against yardstick A ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_car", [True, False], ids=["car", "nocar"])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_modes_against_the_oracle(ffi, SB, small, blend, with_car):
    bev = gen(SB, blend=blend)
    car = small.car if with_car else None
    hs, want = small.table("mixed", 5), small.want("mixed", blend, with_car, 5)
    what = "blend %d car %d" % (blend, with_car)
    got, path = MV.run_step(ffi, bev, small.frames[:5], hs, car)
    assert path == ffi.PATH_PER_PIXEL and bev.out_pitch == 256
    MV.assert_images(dense(got), want, small.none, "device entry, " + what)
    host = bev.batch_homographies(small.frames[:5], hs, car)          # bevw_run_homographies: host buffers, dense images
    assert bev.last_path() == ffi.PATH_PER_PIXEL
    MV.assert_images(host, want, small.none, "host entry, " + what)
    static = bev.batch(small.frames[:5], car)                        # ... and the moving images are not the static ones
    assert [np.array_equal(static[b], want[b]) for b in range(5)] == [False] * 4 + [True], what


# ---- 2. every matrix the handle's own ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["tile_plan", "per_pixel"])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_the_handles_own_matrices_give_the_static_step(ffi, SB, small, blend, sched):
    bev = gen(SB, blend=blend, schedule=ffi.SCHED_PER_PIXEL if sched == "per_pixel" else ffi.SCHED_TILE_PLAN)
    hs = MV.table([("own H", small.rig)] * 5)
    want, path = MV.run_step(ffi, bev, small.frames[:5], None, small.car)
    assert path == (ffi.PATH_PER_PIXEL if sched == "per_pixel" else ffi.PATH_UNITS)
    got, path = MV.run_step(ffi, bev, small.frames[:5], hs, small.car)
    assert path == ffi.PATH_PER_PIXEL
    H.assert_equal(dense(got), dense(want), "own H against bevw_run_device on the %s schedule, blend %d" % (sched, blend))


# ---- 3. yardstick B per frame set ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_against_a_fresh_generator_per_frame_set(ffi, SB, small, blend):
    rigs = small.rigs("mixed", 5)
    want = MV.library_images(SB, rigs, small.frames[:5], small.car, blend)
    bev = gen(SB, blend=blend)
    got, _ = MV.run_step(ffi, bev, small.frames[:5], MV.table(rigs), small.car)
    MV.assert_images(dense(got), want, small.none, "yardstick B, blend %d" % blend)


@pytest.mark.parametrize("key,value", [("warp", 21), ("remap", 1)], ids=["compat_warp_21", "compat_remap_1"])
def test_against_a_fresh_generator_under_a_compat_switch(key, value):
    """BEVW_COMPAT_WARP 21 (a float32 member: fp64 coordinates, fused interpolation) and BEVW_COMPAT_REMAP 1 (ties to even), each in a
    process of its own: the switches are process-wide defaults that a handle snapshots at bevw_build."""
    H.run_child("_moving_worker.py", [key, value], timeout=300, expect="worker OK %s %d" % (key, value))


# ---- 4. hostile families -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_hostile_families_against_the_oracle(ffi, SB, small, blend):
    n = len(small.hostile)
    bev = gen(SB, blend=blend)
    want = small.want("hostile", blend, True, n)
    got, path = MV.run_step(ffi, bev, small.frames[:n], small.table("hostile", n), small.car)
    assert path == ffi.PATH_PER_PIXEL
    for b, (name, _) in enumerate(small.hostile):
        H.assert_same(dense(got)[b], want[b], small.none, "%s, blend %d" % (name, blend))
    # one camera alone perturbed: where the front camera does not contribute the image is the static one
    names = [name for name, _ in small.hostile]
    own, alone = names.index("own H"), names.index("front alone")
    static = bev.batch(small.frames[alone:alone + 1], small.car)[0]
    H.assert_equal(dense(got)[own], bev.batch(small.frames[own:own + 1], small.car)[0], "own H is the static image")
    front = np.asarray(O.RefBevGenerator(small.rig, CFG, blend=blend).masks[0]) != 0
    assert front.any() and (~front).any()
    H.assert_equal(dense(got)[alone][~front], static[~front], "front alone: the pixels outside the front mask, blend %d" % blend)
    assert (dense(got)[alone][front] != static[front]).mean() > 0.5


# ---- 5. batches on one handle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_batches_1_17_33_on_one_handle(ffi, SB, small, blend):
    """(run_step overwrites the matrix array with NaN as soon as each call returns, before the sync)"""
    bev = gen(SB, blend=blend)
    for B in (1, 17, 33):
        got, path = MV.run_step(ffi, bev, small.frames[:B], small.table("mixed", B), small.car)
        assert path == ffi.PATH_PER_PIXEL
        MV.assert_images(dense(got), small.want("mixed", blend, True, B), small.none, "batch %d, blend %d" % (B, blend))


def test_consecutive_steps_need_no_host_synchronisation(ffi, SB, small):
    """six steps queued back to back on one handle with six different tables, each array poisoned at once: more than the four staging slots"""
    bev = gen(SB)
    need = bev.out_image_bytes
    d_in = ffi.DeviceBuffer(small.frames[:6].nbytes).upload(small.frames[:6])
    d_out = ffi.DeviceBuffer(6 * need)
    try:
        for b in range(6):
            hs = small.table("mixed", 6)[b:b + 1].copy()
            bev.run_homographies_device(d_in.ptr + b * bev.in_set_bytes, hs, 1, None, d_out.ptr + b * need, out_bytes=need)
            hs[...] = np.nan
        bev.sync()
        got = d_out.download((6, CFG["BEV_HEIGHT"], bev.out_pitch, 3))
        MV.assert_images(dense(got), small.want("mixed", False, False, 6), small.none, "six queued steps")
    finally:
        d_in.free()
        d_out.free()


# ---- 6. output rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch,px", [("dense", 248), ("aligned", 256), (252, 252)], ids=["dense", "aligned", "252"])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_output_rows(ffi, SB, small, blend, pitch, px):
    bev = gen(SB, blend=blend, output_pitch=pitch)
    assert bev.out_pitch == px and bev.out_image_bytes == px * CFG["BEV_HEIGHT"] * 3
    got, path = MV.run_step(ffi, bev, small.frames[:5], small.table("mixed", 5), small.car)   # exactly the batch's bytes between guards
    assert path == ffi.PATH_PER_PIXEL and got.shape == (5, CFG["BEV_HEIGHT"], px, 3)
    assert (got[:, :, BW:] == MV.FILL).all(), "the padding columns are not written"
    MV.assert_images(dense(got), small.want("mixed", blend, True, 5), small.none, "rows of %d, blend %d" % (px, blend))
    host = bev.batch_homographies(small.frames[:5], small.table("mixed", 5), small.car)       # the host entry compacts the rows
    MV.assert_images(host, small.want("mixed", blend, True, 5), small.none, "rows of %d, blend %d, host entry" % (px, blend))


# ---- 7. addresses ----------------------------------------------------------------------------------------------------------------------------
def test_misaligned_buffers_are_served_on_a_dense_handle(ffi, SB, small):
    bev = gen(SB, blend=True, output_pitch="dense")
    hs, want = small.table("mixed", 5), small.want("mixed", True, True, 5)
    for kw in (dict(off_frames=1), dict(off_out=2), dict(off_car=1), dict(off_frames=3, off_out=1, off_car=2)):
        got, path = MV.run_step(ffi, bev, small.frames[:5], hs, small.car, **kw)
        assert path == ffi.PATH_PER_PIXEL, kw
        MV.assert_images(got, want, small.none, "dense handle, %s" % kw)
        got, path = MV.run_step(ffi, bev, small.frames[:5], hs, small.car)
        MV.assert_images(got, want, small.none, "dense handle, the next aligned step after %s" % kw)


def test_a_pitched_handle_refuses_a_misaligned_step_and_writes_nothing(ffi, SB, small):
    bev = gen(SB, output_pitch="aligned")
    hs = small.table("mixed", 2)
    got, path = MV.run_step(ffi, bev, small.frames[:2], None, small.car)
    assert path == ffi.PATH_UNITS
    for kw in (dict(off_frames=1), dict(off_out=2), dict(off_car=1)):
        with pytest.raises(ffi.BevwError, match="bevw_run_homographies_device.*4-byte aligned"):
            MV.run_step(ffi, bev, small.frames[:2], hs, small.car, **kw)   # (raises only after it found the guards and the batch's bytes untouched)
        assert bev.last_path() == ffi.PATH_UNITS   # a refused step leaves it unchanged
    got, path = MV.run_step(ffi, bev, small.frames[:2], hs, small.car)
    assert path == ffi.PATH_PER_PIXEL
    MV.assert_images(dense(got), small.want("mixed", False, True, 2), small.none, "pitched handle, aligned")


# ---- 8. other geometries ---------------------------------------------------------------------------------------------------------------------
def _geometry(ffi, SB, rig, cfg, blend, frames, car, what, **kw):
    rigs = [MV.mixed_rigs(O, rig, cfg)[i] for i in (1, 3, 4, 0, 2)][:frames.shape[0]]   # pitch -2, roll 1, own H, pitch +0.5, yaw 1
    want, none = MV.oracle_images(O, rigs, frames, car, blend, cfg)
    bev = gen(SB, rig=rig, cfg=cfg, blend=blend, **kw)
    got, path = MV.run_step(ffi, bev, frames, MV.table(rigs), car)
    assert path == ffi.PATH_PER_PIXEL
    MV.assert_images(dense(got, cfg["BEV_WIDTH"]), want, none, what)
    return bev


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_bev_width_250(ffi, SB, blend):
    cfg = dict(CFG, BEV_WIDTH=250)
    rng = np.random.default_rng(1803)
    for pitch in ("dense", "aligned"):
        _geometry(ffi, SB, H.small_rig(), cfg, blend, MV.frames_for(rng, 3, cfg), H.random_car(rng, cfg), "BEV_WIDTH 250, %s rows, blend %d" % (pitch, blend),
                  output_pitch=pitch)


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_frames_of_322_by_258(ffi, SB, blend):
    cfg = dict(CFG, FRAME_WIDTH=322, FRAME_HEIGHT=258)
    rng = np.random.default_rng(1804)
    _geometry(ffi, SB, H.small_rig(), cfg, blend, MV.frames_for(rng, 3, cfg), H.random_car(rng, cfg), "322 x 258 frames, blend %d" % blend)


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_a_bev_without_a_car(ffi, SB, blend):
    cfg = SC.geo_cfg((252, 180, 0, 0))
    rng = np.random.default_rng(1805)
    bev = _geometry(ffi, SB, H.small_rig(), cfg, blend, MV.frames_for(rng, 3, cfg), None, "no car, blend %d" % blend)
    assert not bev.plan_info()["plan_usable"], "more than two contributors on some pixel"


@pytest.mark.parametrize("seed", [1, 2, 11])   # the first three seeds of the fuzz without balance
def test_random_rig_cases(ffi, SB, seed):
    case = H.random_rig_case(seed)
    assert not case["balance"]
    _geometry(ffi, SB, case["rig"], case["cfg"], case["blend"], case["frames"], case["car"], "random rig case %d" % seed, schedule=case["schedule"])


# ---- 9. the static step afterwards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_the_static_step_is_back_on_the_units_with_its_bytes(ffi, SB, small, blend):
    bev = gen(SB, blend=blend)
    L, h = ffi.lib(), bev._engine.h
    assert L.bevw_last_path(h) == ffi.PATH_NONE
    tables = [np.empty((BW * CFG["BEV_HEIGHT"], 2), np.int16) for _ in range(2)]
    codes = [np.empty(BW * CFG["BEV_HEIGHT"], np.uint16) for _ in range(2)]
    ffi.check(L.bevw_get_lut(h, 0, ffi.ptr(tables[0]), ffi.ptr(codes[0])))
    before, path = MV.run_step(ffi, bev, small.frames[:5], None, small.car)
    assert path == ffi.PATH_UNITS
    _, path = MV.run_step(ffi, bev, small.frames[:5], small.table("hostile", 5), small.car)
    assert path == ffi.PATH_PER_PIXEL and L.bevw_last_path(h) == ffi.PATH_PER_PIXEL
    after, path = MV.run_step(ffi, bev, small.frames[:5], None, small.car)
    assert path == ffi.PATH_UNITS and L.bevw_last_path(h) == ffi.PATH_UNITS
    H.assert_equal(after, before, "bevw_run_device after a moving step, blend %d" % blend)
    ffi.check(L.bevw_get_lut(h, 0, ffi.ptr(tables[1]), ffi.ptr(codes[1])))
    H.assert_equal(tables[1], tables[0], "the handle's own BEV table of the front camera")
    H.assert_equal(codes[1], codes[0], "the handle's own fraction codes of the front camera")


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------
def _handle(ffi, before=None, after=None, balance=0, build=True):
    """a raw handle of the small rig: created, `before`(h), cameras set and built, `after`(h)"""
    L = ffi.lib()
    cfg = ffi.bevw_config(CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"], BW, CFG["BEV_HEIGHT"], 62, 100, 1.0, 2.0, balance, balance, 0, 0)
    h = C.c_void_p()
    ffi.check(L.bevw_create(C.byref(cfg), C.byref(h)))
    try:
        if before:
            ffi.check(before(h))
        for i, n in enumerate(MV.CAMERAS):
            K, D, Hm = H.small_rig()[n]
            ffi.check(L.bevw_set_camera(h, i, ffi.ptr(ffi.f64(K, 9)), ffi.ptr(ffi.f64(D, 4)), ffi.ptr(ffi.f64(Hm, 9))))
        if build:
            ffi.check(L.bevw_build(h))
        if after:
            ffi.check(after(h))
    except Exception:
        L.bevw_destroy(h)
        raise
    return h


def test_refusals_in_both_orders(ffi, small):
    L = ffi.lib()
    cams = np.array([0, 1], np.int32)
    hs = small.table("mixed", 1)
    frames = np.ascontiguousarray(small.frames[:1])
    nv12_pitch = lambda h: L.bevw_set_input_format(h, ffi.INPUT_NV12) or L.bevw_set_input_pitch(h, CFG["FRAME_WIDTH"] + 4)
    setters = [(lambda h: L.bevw_set_input_format(h, ffi.INPUT_NV12), b"input format"), (lambda h: L.bevw_set_input_format(h, ffi.INPUT_YUYV), b"input format"),
               (lambda h: L.bevw_set_input_format(h, ffi.INPUT_UYVY), b"input format"), (lambda h: L.bevw_set_output_format(h, ffi.OUTPUT_NV12), b"BEVW_OUTPUT_NV12"),
               (lambda h: L.bevw_set_channels(h, 1), b"1 channel"), (nv12_pitch, b"input format"),
               (lambda h: L.bevw_set_projection(h, ffi.PROJ_ANALYTIC), b"analytic"), (lambda h: L.bevw_set_projection(h, ffi.PROJ_ANALYTIC_F32), b"analytic"),
               (lambda h: L.bevw_set_camera_shard(h, ffi.ptr(cams), 2), b"camera-shard")]
    d_in = ffi.DeviceBuffer(frames.nbytes).upload(frames)
    d_out = ffi.DeviceBuffer(2 * 256 * CFG["BEV_HEIGHT"] * 3)
    out = np.full((1, CFG["BEV_HEIGHT"], BW, 3), MV.FILL, np.uint8)

    def refused(h, word, what):
        d_out.fill(MV.FILL)
        for name, call in ((ENTRY, lambda: L.bevw_run_homographies_device(h, d_in.ptr, ffi.ptr(hs), 1, None, d_out.ptr)),
                           (b"bevw_run_homographies", lambda: L.bevw_run_homographies(h, ffi.ptr(frames), ffi.ptr(hs), 1, None, ffi.ptr(out)))):
            status = call()
            err = L.bevw_last_error()
            assert status == -1 and err.startswith(name + (b":" if b"bevw_build" in word else b" is not available with")) and word in err, (what, name, status, err)
        L.bevw_sync(h)
        assert (d_out.download((d_out.nbytes,)) == MV.FILL).all() and (out == MV.FILL).all(), "%s: a refused step wrote something" % what

    try:
        for k, (setter, word) in enumerate(setters):
            for order in ("before", "after"):
                h = _handle(ffi, **{order: setter})
                try:
                    refused(h, word, "setter %d %s bevw_build" % (k, order))
                finally:
                    L.bevw_destroy(h)
        h = _handle(ffi, balance=1)
        try:
            refused(h, b"balance", "a balance handle")
        finally:
            L.bevw_destroy(h)
        h = _handle(ffi, build=False)
        try:
            refused(h, b"bevw_build has not been called", "an unbuilt handle")
        finally:
            L.bevw_destroy(h)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_a_matrix_that_is_not_finite_is_refused_with_nothing_written(ffi, SB, small, bad):
    bev = gen(SB)
    L, h = ffi.lib(), bev._engine.h
    hs = small.table("mixed", 3)
    hs[2, 1, 1, 2] = bad
    frames = np.ascontiguousarray(small.frames[:3])
    d_in = ffi.DeviceBuffer(frames.nbytes).upload(frames)
    d_out = ffi.DeviceBuffer(3 * bev.out_image_bytes)
    out = np.full((3, CFG["BEV_HEIGHT"], BW, 3), MV.FILL, np.uint8)
    try:
        d_out.fill(MV.FILL)
        for status in (L.bevw_run_homographies_device(h, d_in.ptr, ffi.ptr(hs), 3, None, d_out.ptr),
                       L.bevw_run_homographies(h, ffi.ptr(frames), ffi.ptr(hs), 3, None, ffi.ptr(out))):
            err = L.bevw_last_error()
            assert status == -1 and b"frame set 2, camera 1" in err and b"not finite" in err and b"bevw_run_homographies" in err, (status, err)
        bev.sync()
        assert (d_out.download((d_out.nbytes,)) == MV.FILL).all() and (out == MV.FILL).all(), "a refused step wrote something"
        assert bev.last_path() == ffi.PATH_NONE
        with pytest.raises(Exception, match="frame set 2, camera 1"):
            bev.batch_homographies(frames, hs)
    finally:
        d_in.free()
        d_out.free()
    # a finite matrix whose INVERSE is not: the determinant underflows to a subnormal, its reciprocal is infinite
    tiny = small.table("mixed", 1)
    tiny[0, 3] = np.diag([1e-160, 1e-160, 1.0])
    status = L.bevw_run_homographies(h, ffi.ptr(frames), ffi.ptr(tiny), 1, None, ffi.ptr(out))
    err = L.bevw_last_error()
    assert status == -1 and b"frame set 0, camera 3" in err and b"inverse" in err, (status, err)
    assert (out == MV.FILL).all()
