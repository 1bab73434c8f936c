"""The batch loop of the kernels that came after tests/test_batch_chunks_gpu.py, on the GPU: k_units_gray, k_units_gray16, k_units_nn8 /
k_units_nn16 and k_stitch_units_gray (mono_unit_run, the one-channel form of plan_unit_run's frame loop) with their per-tap kernels, k_units_yuv422 /
k_units_out_yuv422 (the shared loop, instantiated with 16-byte group loads) and k_stitch_moving (a loop and a chunk rule of its own).

tests/_batch_loops.py has the cases, pools and yardsticks; tests/test_batch_chunks_gpu.py says what a wrong frame_of() clamp does and why
the batches of H.BATCHES run in that order on one handle.  Every frame of a pool is distinct, every image of every batch is compared at
tolerance 0 after a 0x5A fill of the whole output buffer, the image-sized guard behind image B - 1 must keep the fill, and every step
asserts its path: the units (the moving step: PATH_PER_PIXEL, which is what the library reports for k_stitch_moving -- it has no other
kernel).  A failure names the batch, the frame, its chunk and whether it is the chunk's last frame.  Expected images are computed once per
module.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest

from tests import _batch_loops as BL
from tests import _harness as H
from tests._harness import SB, ffi  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = H.SMALL_CFG


# ---------------------------------------------------------------------------------------------------------------
# 1. the four one-channel remappers through bevw_remap_device
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remap_case(ffi, oracle):
    """per depth the pool on the device, per (interpolation, depth) the yardstick's images"""
    maps = BL.remap_maps()
    frames = {d: BL.remap_frames(d) for d in (8, 16)}
    want = {(kind, d): BL.remap_want(oracle, kind, frames[d], maps) for kind, d in BL.REMAPPERS}
    for w, fixed in want.values():
        assert fixed.any() and not w[:, fixed].any()
    dev = {d: ffi.DeviceBuffer(f.nbytes).upload(f) for d, f in frames.items()}
    yield frames, want, dev
    for d in dev.values():
        d.free()


@pytest.mark.parametrize("kind,depth", BL.REMAPPERS, ids=["%s%d" % r for r in BL.REMAPPERS])
def test_remapper_ragged_batches(ffi, remap_case, kind, depth):
    _, want, dev = remap_case
    BL.run_remapper(ffi, kind, depth, dev[depth], want[(kind, depth)], H.BATCHES)


# ---------------------------------------------------------------------------------------------------------------
# 2. BevGenerator(channels=1)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gray_case(ffi, oracle):
    frames, car = BL.gray_pool()
    want = {blend: BL.gray_want(oracle, frames, car, blend) for blend in (False, True)}
    d_in, d_car = ffi.DeviceBuffer(frames.nbytes).upload(frames), ffi.DeviceBuffer(car.nbytes).upload(car)
    yield frames, car, want, d_in, d_car
    d_in.free()
    d_car.free()


@pytest.mark.parametrize("pitch,px", [("auto", 256), ("dense", 248)])
@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_gray_stitch_ragged_batches(ffi, SB, gray_case, blend, pitch, px):
    _, car, want, d_in, d_car = gray_case
    bev = BL.run_gray_stitch(ffi, SB, d_in, d_car, car, want[blend], blend, H.BATCHES, output_pitch=pitch)
    assert bev.out_pitch == px


def test_gray_stitch_bev_width_250_pitched(ffi, SB, oracle, gray_case):
    """bw % 4 == 2 on rows of 256: plan_gray_stitch_step copies the car sprite to the images' pitch (pad_car_gray) before every step."""
    frames, _, _, d_in, _ = gray_case
    cfg = dict(CFG, BEV_WIDTH=250)
    car = BL.GS.gray_car(np.random.default_rng(2115), cfg)
    want = BL.gray_want(oracle, frames[:63], car, True, cfg)
    d_car = ffi.DeviceBuffer(car.nbytes).upload(car)
    try:
        bev = BL.run_gray_stitch(ffi, SB, d_in, d_car, car, want, True, (63, 9, 31), cfg=cfg, output_pitch="aligned")
        assert bev.out_pitch == 256
    finally:
        d_car.free()


# ---------------------------------------------------------------------------------------------------------------
# 3. YUYV / UYVY frames through the stitch
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yuv_case(ffi, oracle):
    raw, car = BL.yuv422_pool()
    inputs = H.Inputs(ffi, raw, None, car, yuv422={"yuyv": raw, "uyvy": raw})
    expected = {order: H.Expected(oracle, BL.yuv422_bgr(raw, order), car, CFG, BL.POOL) for order in ("yuyv", "uyvy")}
    yield inputs, expected
    inputs.free()


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("order", ["yuyv", "uyvy"])
def test_yuv422_stitch_ragged_batches(ffi, SB, yuv_case, order, out, blend):
    inputs, expected = yuv_case
    bev = H.stitch_handle(ffi, SB, inputs, expected[order](blend, False), order, out, blend, False)
    assert bev.last_path() == ffi.PATH_UNITS and bev.out_pitch == 256


# ---------------------------------------------------------------------------------------------------------------
# 4. k_stitch_moving
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moving_case(ffi, oracle):
    rigs = BL.moving_rigs(oracle)
    frames, car = BL.moving_pool()
    table = BL.MV.table([rigs[b % len(rigs)] for b in range(BL.MOVING_POOL)])
    d_in, d_car = ffi.DeviceBuffer(frames.nbytes).upload(frames), ffi.DeviceBuffer(car.nbytes).upload(car)
    yield rigs, frames, car, table, d_in, d_car
    d_in.free()
    d_car.free()


@pytest.mark.parametrize("blend", [False, True], ids=["direct", "blend"])
def test_moving_ragged_blocks(ffi, SB, oracle, moving_case, blend):
    """Batches 67, 131 and 259 on 252 tiles: blocks of 4, 8 and 16 frame sets with a last block of 3 (BL.MOVING, held against moving_nb on
    the host); then 33 and 9 on the same handle.  The matrix array is overwritten with NaN as soon as each call returns."""
    rigs, frames, car, table, d_in, d_car = moving_case
    cfg = BL.MOVING_CFG
    want = BL.moving_want(oracle, rigs, frames, car, blend)
    assert len({w.tobytes() for w in want[0][:14]}) == 14
    bev = H.generator(SB, BL.FB.scaled_rig(cfg), cfg, blend=blend)
    assert (cfg["BEV_WIDTH"] + 63) // 64 * ((cfg["BEV_HEIGHT"] + 3) // 4) == BL.MOVING_TILES
    what = "moving, blend %d" % blend

    def launch(B, d_out):
        hs = np.array(table[:B], np.float64)
        bev.run_homographies_device(d_in.ptr, hs, B, d_car.ptr, d_out.ptr, out_bytes=d_out.nbytes)
        hs[...] = np.nan

    def sync():
        bev.sync()
        assert bev.last_path() == ffi.PATH_PER_PIXEL, "%s: path %d" % (what, bev.last_path())

    H.run_batches(ffi, launch, sync, bev.out_image_bytes, False, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], bev.out_pitch, BL.MOVING_BATCHES, want, what,
                  nb_env={B: v[0] for B, v in BL.MOVING.items()})


# ---------------------------------------------------------------------------------------------------------------
# 5. the launch-map switches, each in a fresh child (the library reads BEVW_PLAN_* once per process)
# ---------------------------------------------------------------------------------------------------------------
SWITCHES = {"xcdmap2": ("BEVW_PLAN_XCDMAP", "2"), "xcdmap0": ("BEVW_PLAN_XCDMAP", "0"), "nb5": ("BEVW_PLAN_NB", "5")}
# seconds: a child measured 0.98 .. 1.07 s of wall time (profiles/f21_batch_loops/durations.txt); five times that lies under the floor of 60 s that the
# far-batch children get, and the margin covers a cold code-object load and a busy shared box
CHILD_TIMEOUT = 60


@pytest.fixture(scope="module")
def case_dir(remap_case, gray_case, yuv_case, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_loops"))
    frames, want, _ = remap_case
    files = {"frames%d" % depth: f for depth, f in frames.items()}
    for (kind, depth), (w, fixed) in want.items():
        files["want_%s%d" % (kind, depth)], files["fixed_%s%d" % (kind, depth)] = w, fixed
    gray, gray_car, gray_want, _, _ = gray_case
    files["gray"], files["gray_car"] = gray, gray_car
    for blend, (w, none) in gray_want.items():
        files["gray_want%d" % blend], files["gray_none%d" % blend] = w, none
    inputs, expected = yuv_case
    w, _, none = expected["yuyv"](True, False)
    files.update(yuyv=inputs.nv, car=inputs.car.download(w[0].shape), yuyv_want=w, yuyv_none=none)
    for name, a in files.items():
        np.save(os.path.join(d, name + ".npy"), a)
    return d


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_launch_map_switches(case_dir, switch):
    name, value = SWITCHES[switch]
    H.run_child("_batch_loops_worker.py", [case_dir, name, value], {name: value}, ("BEVW_PLAN_",), CHILD_TIMEOUT, "worker OK %s=%s" % (name, value))
