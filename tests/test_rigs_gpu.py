"""The rig catalogue (tests/_rigs.py) through bevw_build and bevw_run* on the GPU: rigs that are no variation of the sample rig.

A calibration reaches the device through bevw_set_camera only; the table builders (k_fisheye_map: fp64 sqrt / atan against the host's libm;
k_bev_lut: perspective_coord with its saturations, the LUT quirk), the plan compile on the device-built tables (k_plan_build, the unit
compiler, the per-tap kernel's border tiles, the balance's group lists) and the analytic kernels are all functions of it.  Per family:
  * tables     undistort maps, LUTs and masks of all four cameras equal the oracle's -- first, so that a wrong image can be traced to a
               builder or to a frame kernel;
  * stitch     the four (blend, balance) modes on the per-pixel schedule and on AUTO (which must pick the tile plan), tolerance 0 against
               oracle.RefBevGenerator, the two schedules equal; the units take at least the share the host emulator gives them
               (_rigs.UNIT_FLOOR, tests/test_rigs_host.py), and on _rigs.BORDER the per-tap kernel serves border tiles (tiles_border > 0: by
               plan_stitch's dispatch, k_stitch_plan runs on the base tiles no unit owns);
  * on _rigs.METHODS: Camera.raw2bev / undistort / warp_homography, and NV12 in, YUYV in, BGR -> NV12 out against the specifications of the
    format tests (tests/_nv12_spec.py, _yuv422_spec.py, _nv12_out_spec.py);
  * on _rigs.ANALYTIC: projection="analytic" against np_analytic.AnalyticBevGenerator at the bars of tests/_analytic_common.py.
Batch 3, random frames, camera 1 at half brightness (non-trivial luminance deltas), a random car sprite; images are written into a buffer
filled with 0x5A with a guard behind it (_analytic_common.stitch_filled), the pixels no camera covers are asserted by name first.
Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from tests import _analytic_common as AC
from tests import _harness as H
from tests import _nv12_spec as SN
from tests import _rigs as R
from tests import _yuv422_spec as SY
from tests._analytic_common import check_batch
from tests._harness import SB, assert_nv12, assert_same, ffi, uncovered  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH = 3
MODES = {"direct": (False, False), "blend": (True, False), "balance": (False, True), "blend_balance": (True, True)}


_frames, _wants = {}, {}


def inputs(cfg):
    """(frames [BATCH, 4, FH, FW, 3], car) of a geometry, made once"""
    key = (cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"])
    if key not in _frames:
        _frames[key] = (R.frames(cfg, BATCH), R.car(cfg))
    return _frames[key]


def expected(name, blend, balance):
    """(oracle images of inputs() [BATCH], pixels no camera covers), computed once per (family, mode)"""
    key = (name, blend, balance)
    if key not in _wants:
        ref = R.ref(name, blend, balance)
        frames, car = inputs(ref.cfg)
        none = uncovered(ref)
        assert none.any(), "the rig has pixels no camera covers"
        _wants[key] = ([ref(*frames[b], car) for b in range(BATCH)], none)
    return _wants[key]


def generator(SB, name, **kw):
    return H.generator(SB, *R.family(name), **kw)


# ---------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
def test_tables(ffi, SB, oracle, name):
    for blend in (False, True):
        bev, ref = generator(SB, name, blend=blend), R.ref(name, blend)
        for i, n in enumerate(R.CAMS):
            if not blend:
                u1, u2 = bev.cameras[i].undistort_maps
                w1, w2 = ref.cameras[i].undistort_maps
                assert u1.shape == w1.shape and np.array_equal(u1, w1), "%s %s: undistort map1, %d entries differ" % (name, n, int((u1 != w1).any(-1).sum()))
                assert np.array_equal(u2, w2), "%s %s: undistort map2, %d entries differ" % (name, n, int((u2 != w2).sum()))
                b1, b2 = bev.cameras[i].bev_maps
                assert np.array_equal(b1, ref.cameras[i].bev_maps[0]), "%s %s: bev map1, %d entries differ" % (
                    name, n, int((b1 != ref.cameras[i].bev_maps[0]).any(-1).sum()))
                assert np.array_equal(b2, ref.cameras[i].bev_maps[1]), "%s %s: bev map2, %d entries differ" % (
                    name, n, int((b2 != ref.cameras[i].bev_maps[1]).sum()))
            assert np.array_equal(bev.masks[i].mask, ref.masks[i]), "%s %s: mask, blend=%s" % (name, n, blend)


# ---------------------------------------------------------------------------------------------------------------
# stitch at tolerance 0, both schedules
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", R.FAMILIES)
def test_stitch(ffi, SB, oracle, name, mode):
    blend, balance = MODES[mode]
    want, none = expected(name, blend, balance)
    frames, car = inputs(R.family(name)[1])
    outs = {}
    for schedule in (ffi.SCHED_PER_PIXEL, ffi.SCHED_AUTO):
        bev = generator(SB, name, blend=blend, balance=balance, schedule=schedule, output_pitch="dense")
        info = bev.plan_info()
        if schedule == ffi.SCHED_AUTO:
            assert info["schedule"] == ffi.SCHED_TILE_PLAN == 2 and info["plan_usable"], info
            share = info["tiles_staged"] / float(info["tiles_x"] * info["tiles_y"])
            print("%s %s: %d of %d x %d base tiles on the units (%.4f, host floor %.2f), %d border tiles" % (
                name, mode, info["tiles_staged"], info["tiles_x"], info["tiles_y"], share, R.UNIT_FLOOR[name][blend], info["tiles_border"]))
            assert share >= R.UNIT_FLOOR[name][blend], "%s: the units take %.4f of the base tiles, host floor %.2f" % (name, share, R.UNIT_FLOOR[name][blend])
            if name in R.BORDER:
                assert info["tiles_border"] > 0, "%s: no border tile for the per-tap kernel" % name
        else:
            assert info["schedule"] == ffi.SCHED_PER_PIXEL
        got = AC.stitch_filled(ffi, bev, frames, car)
        for b in range(BATCH):
            assert_same(got[b], want[b], none, "%s %s, schedule %d, image %d" % (name, mode, info["schedule"], b))
        outs[schedule] = got
    assert np.array_equal(outs[ffi.SCHED_PER_PIXEL], outs[ffi.SCHED_AUTO])
    # the default device layout (rows of whole sectors) through the host entry point
    bev = generator(SB, name, blend=blend, balance=balance)
    assert bev.out_pitch == 256 and bev.plan_info()["schedule"] == ffi.SCHED_TILE_PLAN
    got = bev.batch(frames, car)
    for b in range(BATCH):
        assert_same(got[b], want[b], none, "%s %s, rows of whole sectors, image %d" % (name, mode, b))


# ---------------------------------------------------------------------------------------------------------------
# Camera methods
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.METHODS)
def test_camera_methods(ffi, SB, oracle, name):
    """camera 0 as the reference's demo uses it -- and the other three, which on these rigs are different cameras"""
    bev, ref = generator(SB, name), R.ref(name)
    for i, n in enumerate(R.CAMS):
        frame = inputs(ref.cfg)[0][0, i]
        got, want = bev.cameras[i].raw2bev(frame), ref.cameras[i].raw2bev(frame)
        assert np.array_equal(got, want), "%s %s: raw2bev, %d pixels differ" % (name, n, int((got != want).any(-1).sum()))
        und, wund = bev.cameras[i].undistort(frame), ref.cameras[i].undistort(frame)
        assert und.shape == wund.shape and np.array_equal(und, wund), "%s %s: undistort, %d pixels differ" % (name, n, int((und != wund).any(-1).sum()))
        got, want = bev.cameras[i].warp_homography(wund), ref.cameras[i].warp_homography(wund)
        assert np.array_equal(got, want), "%s %s: warp_homography, %d pixels differ" % (name, n, int((got != want).any(-1).sum()))


# ---------------------------------------------------------------------------------------------------------------
# pixel formats
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12_in", "yuyv_in", "nv12_out"])
@pytest.mark.parametrize("mode", ["direct", "blend_balance"])
@pytest.mark.parametrize("name", R.METHODS)
def test_formats(ffi, SB, oracle, name, mode, fmt):
    blend, balance = MODES[mode]
    ref = R.ref(name, blend, balance)
    cfg = ref.cfg
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    none = uncovered(ref)
    assert none.any()
    car = inputs(cfg)[1]
    rng = np.random.default_rng([R.FAMILIES.index(name), blend, ["nv12_in", "yuyv_in", "nv12_out"].index(fmt)])
    if fmt == "nv12_in":
        frames = SN.random_nv12(rng, (BATCH, 4), fw, fh)
        frames[:, 1, :fh] //= 2                    # camera 1 at half brightness: the Y plane
        bgr = [SN.nv12_to_bgr(f) for f in frames]
        kw = dict(input_format="nv12")
    elif fmt == "yuyv_in":
        frames = SY.random_yuv422(rng, (BATCH, 4), fw, fh)
        frames[:, 1, :, :, 0] //= 2                # YUYV: Y is the first byte of every texel
        bgr = SY.yuv422_to_bgr(frames, "yuyv")
        kw = dict(input_format="yuyv")
    else:
        frames = inputs(cfg)[0]
        bgr = list(frames)
        kw = dict(output_format="nv12")
    bev = generator(SB, name, blend=blend, balance=balance, **kw)
    info = bev.plan_info()
    assert info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] / float(info["tiles_x"] * info["tiles_y"]) >= R.UNIT_FLOOR[name][blend]
    got = bev.batch(frames, car)
    for b in range(BATCH):
        want = ref(*bgr[b], car)
        what = "%s %s %s, image %d" % (name, mode, fmt, b)
        if fmt == "nv12_out":
            assert_nv12(got[b], want, none, what, black=False)
        else:
            assert_same(got[b], want, none, what)


# ---------------------------------------------------------------------------------------------------------------
# analytic projection
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", R.ANALYTIC)
def test_analytic(ffi, SB, oracle, name, mode):
    blend, balance = MODES[mode]
    assert name in AC.RIGS and R.family(name)[1] == AC.SMALL_CFG
    frames, car = AC.make_frames(BATCH, cast=balance), AC.make_car()   # balance: the colour cast that keeps the gains far from 1
    bev = generator(SB, name, blend=blend, balance=balance, projection="analytic")
    got = AC.stitch_filled(ffi, bev, frames, car)
    left = bev.plan_info()["analytic_tiles_left"]
    print("%s %s: base tiles left to k_stitch_analytic: %d" % (name, mode, left))
    assert left == -1 if balance else left >= 0     # balance: the full-grid kernel; otherwise the wide unit plan is in use
    check_batch(got, AC.spec(name, AC.SMALL_CFG, blend, balance), frames, car, balance, "%s %s" % (name, mode))
