"""What the GPU tests share: the `ffi` / `SB` fixtures, the small rig and its generators, the tolerance-0 assertions, the ctypes Remapper,
the device-resident pool and batch runner of the batch-loop tests, and the launcher of worker processes.

No test module is imported from here and none imports another: helpers and workers reach this file as `tests._harness`.  The library is
loaded inside the functions that need it, never at import, so host tests may import this file on a machine without the built library.

run_child() is the one launcher of tests/_*_worker.py children.  A child that fails an assertion fails the test; a child that ran into
its time limit, was killed by a signal or exited with 134 / 139 / 124 / 137 ends the whole pytest session, because after a GPU fault or
hang nothing more may start on that GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _nv12_out_spec as SO
from tests import _nv12_surfaces as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# fixtures (pulled in with `from tests._harness import ffi, SB  # noqa: F401`)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ffi():
    from cameracalibration_amd import _ffi

    _ffi.require_device()
    return _ffi


@pytest.fixture(scope="module")
def SB():
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV

    return surroundBEV


# ---------------------------------------------------------------------------------------------------------------
# the small rig: the repo rig scaled to 320 x 256 frames -> 248 x 250 BEV, a geometry that exercises every path quickly
# ---------------------------------------------------------------------------------------------------------------
SMALL_CFG = dict(FRAME_WIDTH=320, FRAME_HEIGHT=256, BEV_WIDTH=248, BEV_HEIGHT=250, CAR_WIDTH=62, CAR_HEIGHT=100,
                 FOCAL_SCALE=1.0, SIZE_SCALE=2.0)


def small_rig():
    from cameracalibration_amd import workloads as W

    A = np.diag([0.25, 0.25, 1.0])   # raw frame, undistorted grid and BEV all scale by 1/4: H_s = A . H . A^-1
    return {n: (A @ K, D.copy(), A @ H @ np.linalg.inv(A)) for n, (K, D, H) in W.repo_rig().items()}


def set_args(SB, cfg):
    ns = SB.BevGenerator.get_args()
    for k, v in cfg.items():
        setattr(ns, k, v)


def generator(SB, rig, cfg, **kw):
    """BevGenerator of a rig at cfg (left in the shared arguments); kw: blend, balance, schedule, projection, the formats and pitches."""
    set_args(SB, cfg)
    return SB.BevGenerator(rig=rig, **kw)


def uncovered(ref):
    """BEV pixels whose masks are all zero: no camera contributes there."""
    return np.all([np.asarray(m) == 0 for m in ref.masks], axis=0)


def outside_of(m1, sw, sh):
    """Pixels whose whole 2 x 2 footprint lies outside the frame."""
    return (m1[..., 0] < -1) | (m1[..., 0] >= sw) | (m1[..., 1] < -1) | (m1[..., 1] >= sh)


def random_car(rng, cfg):
    car = np.zeros((cfg["BEV_HEIGHT"], cfg["BEV_WIDTH"], 3), np.uint8)
    h, w = cfg["CAR_HEIGHT"], cfg["CAR_WIDTH"]
    y0, x0 = (cfg["BEV_HEIGHT"] - h) // 2, (cfg["BEV_WIDTH"] - w) // 2
    car[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return car


def random_rig_case(seed):
    """The seeded geometry fuzz of test_random_rigs_modes_and_batches (shared with tests/test_analytic_gpu.py): frame / BEV / car sizes
    (odd ones included), focal and size scales, modes, batch size, frames, an optional car and a schedule."""
    from cameracalibration_amd import workloads as W

    rng = np.random.default_rng(1000 + seed)
    fw = int(rng.choice([160, 200, 236, 320, 322, 400]))
    fh = int(rng.choice([128, 150, 256, 258]))
    bw = int(rng.choice([96, 124, 125, 200, 248, 250]))
    bh = int(rng.choice([96, 130, 201, 250]))
    cw, ch = int(rng.integers(0, bw // 3 + 1)), int(rng.integers(0, bh // 2 + 1))
    cfg = dict(FRAME_WIDTH=fw, FRAME_HEIGHT=fh, BEV_WIDTH=bw, BEV_HEIGHT=bh, CAR_WIDTH=cw, CAR_HEIGHT=ch,
               FOCAL_SCALE=float(rng.choice([0.8, 1.0, 1.25])), SIZE_SCALE=float(rng.choice([1.0, 1.5, 2.0])))
    # the repo rig scaled to the frame (raw frame by fw/1280, fh/1024) and to the BEV (by bw/1000, bh/1000)
    A = np.diag([fw / 1280.0, fh / 1024.0, 1.0])
    U = np.diag([fw * cfg["SIZE_SCALE"] / 2560.0, fh * cfg["SIZE_SCALE"] / 2048.0, 1.0])   # undistorted grid scale
    Bm = np.diag([bw / 1000.0, bh / 1000.0, 1.0])
    rig = {n: (A @ K, D.copy(), Bm @ H @ np.linalg.inv(U)) for n, (K, D, H) in W.repo_rig().items()}
    blend, balance = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    batch = int(rng.integers(1, 6))
    frames = rng.integers(0, 256, (batch, 4, fh, fw, 3), dtype=np.uint8)
    frames[:, 1] //= 2                       # unequal brightness: non-trivial luminance deltas
    car = None
    if rng.integers(0, 2) and cw and ch:
        car = np.zeros((bh, bw, 3), np.uint8)
        t, l = (bh - ch) // 2, (bw - cw) // 2
        car[t:t + ch, l:l + cw] = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
    schedule = int(rng.choice([0, 0, 1]))
    return dict(cfg=cfg, rig=rig, blend=blend, balance=balance, batch=batch, frames=frames, car=car, schedule=schedule)


def raw_handle(ffi, fw, fh, bw, bh):
    """A bevw handle of the small rig's car and scales at the given frame and BEV sizes, created and nothing else."""
    cfg = ffi.bevw_config(fw, fh, bw, bh, 62, 100, 1.0, 2.0, 0, 0, 0, 0)
    h = C.c_void_p()
    ffi.check(ffi.lib().bevw_create(C.byref(cfg), C.byref(h)))
    return h


SAMPLED = (0, 1, 15, 16, 17, 127, 128, 200, 254, 255)   # frame sets of a batch of 256 checked against the oracle: chunk edges of 16-frame blocks, the ends


def fetch(ffi, bev, d_out, cfg, b):
    """Image b of a device buffer of the generator's images -> dense host array: BGR [BH, BW, 3] or NV12 [BH * 3 // 2, BW]."""
    bh, bw = cfg["BEV_HEIGHT"], cfg["BEV_WIDTH"]
    if bev.output_format == "nv12":
        return d_out.download((bh * 3 // 2, bev.out_pitch), offset=b * bev.out_image_bytes)[:, :bw]
    return d_out.download((bh, bev.out_pitch, 3), offset=b * bev.out_image_bytes)[:, :bw]


def run_table(ffi, bev, table, car, cfg):
    """run_surfaces on a host table [B, 4, 2]; returns the device output buffer (caller frees) after the step finished."""
    B = table.shape[0]
    d_out = ffi.DeviceBuffer(B * bev.out_image_bytes)
    d_out.fill(0x5a)
    d_car = ffi.DeviceBuffer(car.nbytes).upload(car) if car is not None else None
    try:
        bev.run_surfaces(table, d_car.ptr if d_car else None, d_out.ptr, out_bytes=d_out.nbytes)
        bev.sync()
    finally:
        if d_car:
            d_car.free()
    return d_out


# ---------------------------------------------------------------------------------------------------------------
# assertions, all at tolerance 0
# ---------------------------------------------------------------------------------------------------------------
def first_difference(got, want):
    at = np.argwhere(got != want)[0].tolist()
    return "first difference at %s: got %d, want %d" % (at, int(got[tuple(at)]), int(want[tuple(at)]))


def assert_same(got, want, none, what):
    """BGR images [BH, BW, 3]; none: pixels no camera covers, asserted on their own first."""
    assert got.shape == want.shape, what
    bad = np.any(got[none] != want[none], axis=-1)
    assert not bad.any(), "%s: %d pixels no camera covers differ (first %s, got %s want %s) -- a zero tap converted as YUV (0, 0, 0)?" % (
        what, int(bad.sum()), np.argwhere(none)[np.argmax(bad)].tolist(), got[none][bad][0].tolist(), want[none][bad][0].tolist())
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max()) == 0, "%s: max |HIP - oracle| = %d over %d bytes" % (what, int(d.max()), int(np.count_nonzero(d)))


def assert_nv12(got, want_bgr, none, what, black=True):
    """got: NV12 [BH*3//2, BW]; want_bgr: the oracle's BGR image; none: pixels no camera covers (black there unless a car is given)."""
    bh, bw = want_bgr.shape[:2]
    want = SO.bgr_to_nv12(want_bgr)
    assert got.shape == want.shape == (bh * 3 // 2, bw), what
    y, uv = SO.planes(got)
    wy, wuv = SO.planes(want)
    cnone = np.repeat(none[0::2, 0::2], 2, axis=1)   # U / V bytes of blocks whose top-left pixel no camera covers
    bad_y, bad_uv = y[none] != wy[none], uv[cnone] != wuv[cnone]
    assert not bad_y.any() and not bad_uv.any(), (
        "%s: %d Y / %d U,V bytes of pixels no camera covers differ (got Y %s U,V %s, want Y %s U,V %s) -- zeros stored instead of NV12 black?"
        % (what, int(bad_y.sum()), int(bad_uv.sum()), y[none][bad_y][:3].tolist(), uv[cnone][bad_uv][:4].tolist(), wy[none][bad_y][:3].tolist(),
           wuv[cnone][bad_uv][:4].tolist()))
    if black:
        assert (y[none] == 16).all() and (uv[cnone] == 128).all(), what + ": NV12 black is (16, 128, 128)"
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max()) == 0, "%s: max |HIP - spec(oracle)| = %d over %d bytes (Y rows: %s)" % (
        what, int(d.max()), int(np.count_nonzero(d)), sorted(set(np.nonzero(d)[0].tolist()))[:5])


def assert_equal(got, want, what):
    """Any two arrays, no mask."""
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d bytes differ (first at %s)" % (what, int((got != want).sum()), got.size,
                                                                                   tuple(int(i) for i in np.argwhere(got != want)[0]))


def assert_same_gray(got, want, outside, what):
    """One image of a remapper, [DH, DW] or [DH, DW, 3]; outside: pixels whose footprint lies outside the frame, which must be 0."""
    assert got.shape == want.shape and got.dtype == np.uint8, what
    assert not got[outside].any(), "%s: a pixel whose footprint lies outside the frame is not 0" % what
    assert_equal(got, want, what)


def assert_batch_gray(got, want, outside, what):
    assert got.shape == want.shape, what
    for b in range(got.shape[0]):
        assert_same_gray(got[b], want[b], outside, "%s, image %d" % (what, b))


_NOT_GIVEN = object()


def check_image(got, want_bgr, none, what, out="bgr", black=False, car=_NOT_GIVEN, want_nv12=None):
    """One image in format `out` ('bgr' | 'nv12') against the oracle's BGR image, through assert_same / assert_nv12: the pixels no camera
    covers first, by name.  black: those pixels must be NV12 black; car (the sprite of the run, or None), where given, decides it.
    want_nv12: the NV12 form of want_bgr where the caller has it -- then, as for BGR, an image that equals it passes at once and one that
    differs names its first difference before it goes to the assertions."""
    nv12 = out == "nv12"
    if car is not _NOT_GIVEN:
        black = car is None
    want = want_nv12 if nv12 else want_bgr
    if want is not None:
        if got.shape == want.shape and np.array_equal(got, want):
            return
        what = "%s; %s" % (what, first_difference(got, want) if got.shape == want.shape else "shape %s" % (got.shape,))
    if nv12:
        assert_nv12(got, want_bgr, none, what, black=black)
    else:
        assert_same(got, want_bgr, none, what)
    if want is not None:
        raise AssertionError(what)


# ---------------------------------------------------------------------------------------------------------------
# bevw_remapper_from_maps through ctypes
# ---------------------------------------------------------------------------------------------------------------
class Remapper:
    """bevw_remapper_from_maps as a context: the remapper is destroyed on the way out, whatever happened inside (a setter that raises in
    __enter__ included).  maps: (map1, map2) as the caller made them; size: (sw, sh, dw, dh).  inp: an input format to set ('bgr', 'nv12',
    'yuyv', 'uyvy'; None: no call), pitch: an input pitch to set, channels: 1 for a single-channel remapper."""

    def __init__(self, ffi, maps, size, inp=None, pitch=0, channels=3):
        self.ffi, self.L, self.size, self.r = ffi, ffi.lib(), size, C.c_void_p()
        self.m1, self.m2 = maps
        self.inp, self.pitch, self.channels = inp, pitch, channels

    def __enter__(self):
        sw, sh, dw, dh = self.size
        self.ffi.check(self.L.bevw_remapper_from_maps(0, sw, sh, self.ffi.ptr(self.m1), self.ffi.ptr(self.m2), dw, dh, C.byref(self.r)))
        try:
            if self.inp is not None:
                self.ffi.check(self.L.bevw_remapper_set_input_format(self.r, self.ffi.INPUT_FORMATS[self.inp]))
            if self.pitch:
                self.ffi.check(self.L.bevw_remapper_set_input_pitch(self.r, self.pitch))
            if self.channels != 3:
                self.set_channels(self.channels)
        except Exception:
            self.L.bevw_remapper_destroy(self.r)
            raise
        return self

    def __exit__(self, *exc):
        self.L.bevw_remapper_destroy(self.r)
        return False

    def set_channels(self, n):
        self.ffi.check(self.L.bevw_remapper_set_channels(self.r, n))
        assert self.L.bevw_remapper_channels(self.r) == n
        self.channels = n

    def last_path(self):
        return self.L.bevw_remapper_last_path(self.r)

    def set_output(self, out):
        if out is not None:
            self.ffi.check(self.L.bevw_remapper_set_output_format(self.r, self.ffi.OUTPUT_NV12 if out == "nv12" else self.ffi.OUTPUT_BGR))

    def out_shape(self, out, n):
        dw, dh = self.size[2:]
        return (n, dh * 3 // 2, dw) if out == "nv12" else (n, dh, dw) + ((3,) if self.channels == 3 else ())

    def remap(self, frames, out=None):
        """Host frames -> host images over a 0x5a fill.  out: 'bgr' | 'nv12' sets the output format first; None leaves it as it is."""
        self.set_output(out)
        got = np.full(self.out_shape(out, frames.shape[0]), 0x5a, np.uint8)
        self.ffi.check(self.L.bevw_remap(self.r, self.ffi.ptr(np.ascontiguousarray(frames)), frames.shape[0], self.ffi.ptr(got)))
        return got

    def remap_device(self, d_src, batch, d_dst):
        self.ffi.check(self.L.bevw_remap_device(self.r, d_src, batch, d_dst))
        self.ffi.check(self.L.bevw_remapper_sync(self.r))

    def remap_surfaces(self, table, out=None):
        self.set_output(out)
        shape = self.out_shape(out, table.shape[0])
        d_out = self.ffi.DeviceBuffer(int(np.prod(shape)))
        try:
            d_out.fill(0x5a)
            self.ffi.check(self.L.bevw_remap_surfaces_device(self.r, self.ffi.ptr(np.ascontiguousarray(table)), table.shape[0], d_out.ptr))
            self.ffi.check(self.L.bevw_remapper_sync(self.r))
            return d_out.download(shape)
        finally:
            d_out.free()


# ---------------------------------------------------------------------------------------------------------------
# the batch loop: a pool resident on the device, one handle over a list of batch sizes (tests/test_batch_chunks_gpu.py says why)
# ---------------------------------------------------------------------------------------------------------------
BATCHES = (143, 9, 63, 17, 129, 31, 100, 33)   # in this order on one handle
FILL = 0x5A
# batch -> (nb, chunks, frames of the last chunk, XCD map in use, idle chunk slots of the launch) without balance slices ...
PLAIN = {9: (1, 9, 1, 1, 7), 17: (2, 9, 1, 1, 7), 31: (3, 11, 1, 1, 5), 33: (8, 5, 1, 0, 0), 63: (8, 8, 7, 1, 0), 100: (8, 13, 4, 1, 3),
         129: (16, 9, 1, 1, 7), 143: (16, 9, 15, 1, 7)}
# ... and the slices of a balance handle (balance_plan_run, csrc/bevwarp.hip: two from batch 32), each (frames, nb, chunks, last chunk)
SLICES = {9: ((9, 1, 9, 1),), 17: ((17, 2, 9, 1),), 31: ((31, 3, 11, 1),), 33: ((16, 2, 8, 2), (17, 2, 9, 1)),
          63: ((31, 3, 11, 1), (32, 8, 4, 8)), 100: ((50, 8, 7, 2), (50, 8, 7, 2)), 129: ((64, 8, 8, 8), (65, 8, 9, 1)),
          143: ((71, 8, 9, 7), (72, 8, 9, 8))}


WORKER_BATCHES = (143, 17, 63)                                   # what tests/_batch_chunks_worker.py runs, per handle ...
WORKER_MODES = ((False, False), (True, False), (True, True))   # ... packed BGR in, BGR out; and surfaces -> NV12 in the blend mode


def balance_slices(batch):
    """Frame sets per slice of a balance handle's step, as balance_plan_run cuts them."""
    parts = 2 if batch >= 32 else 1
    return [batch * (p + 1) // parts - batch * p // parts for p in range(parts)]


def where(batch, b, balance=False, nb_env=0):
    """'batch B, frame b: chunk c of n frames, last of its chunk or not' -- with the table's nb (nb_env: an explicit BEVW_PLAN_NB, or
    {batch: nb} of a kernel that cuts its batches by a rule of its own: moving_nb)."""
    if isinstance(nb_env, dict):
        nb_env = nb_env[batch]
    slices = [(n, nb) for n, nb, _, _ in SLICES[batch]] if balance else [(batch, PLAIN[batch][0] if batch in PLAIN else nb_env)]
    b0 = 0
    for k, (n, nb) in enumerate(slices):
        nb = min(nb_env, n) if nb_env else nb
        if b < b0 + n:
            i = b - b0
            last = i % nb == nb - 1 or i == n - 1
            return "batch %d, frame %d: %schunk %d (%d frames per chunk), %s of its chunk" % (
                batch, b, "slice %d of %d frames, " % (k, n) if len(slices) > 1 else "", i // nb, nb, "the LAST frame" if last else "not the last frame")
        b0 += n
    raise AssertionError((batch, b))


class Expected:
    """The oracle's images of a pool's frame sets per (blend, balance), computed on first use: .bgr [n, BH, BW, 3], .nv12, .none."""

    def __init__(self, oracle, bgr, car, cfg, n, nv12=True):
        self.oracle, self.frames, self.car, self.cfg, self.n, self.with_nv12, self.cache = oracle, bgr, car, cfg, n, nv12, {}

    def __call__(self, blend, balance):
        key = (bool(blend), bool(balance))
        if key not in self.cache:
            ref = self.oracle.RefBevGenerator(small_rig(), self.cfg, blend=key[0], balance=key[1])
            none = uncovered(ref)
            assert none.any()
            want = np.stack([ref(*self.frames[b], self.car) for b in range(self.n)])
            nv12 = np.stack([SO.bgr_to_nv12(w) for w in want]) if self.with_nv12 else None
            self.cache[key] = (want, nv12, none)
        return self.cache[key]


class Inputs:
    """A pool of SMALL_CFG frame sets resident on the device once per input kind: packed BGR, packed NV12, NV12 surfaces at pitch FW + 4
    with their table, and (yuv422: {'yuyv': frames, 'uyvy': frames}) the packed 4:2:2 forms of a pool that has them."""

    def __init__(self, ffi, nv, bgr, car, cams=4, yuv422=None):
        self.ffi, self.nv, self.bgr, self.cams, self.bufs, self.surf, self.yuv422 = ffi, nv, bgr, cams, {}, None, yuv422 or {}
        self.car = ffi.DeviceBuffer(car.nbytes).upload(car) if car is not None else None

    def host(self, kind):
        return self.bgr if kind == "bgr" else self.yuv422[kind] if kind in self.yuv422 else self.nv

    def packed(self, kind):
        if kind not in self.bufs:
            host = self.host(kind)
            self.bufs[kind] = self.ffi.DeviceBuffer(host.nbytes).upload(host)
        return self.bufs[kind]

    def table(self):
        if self.surf is None:
            fw, fh = SMALL_CFG["FRAME_WIDTH"], SMALL_CFG["FRAME_HEIGHT"]
            self.surf = SF.Surfaces(self.ffi, self.nv.reshape(-1, fh * 3 // 2, fw), fw, fh, fw + 4, layout_seed=51, fill_seed=52, mode="shuffled")
            self.bufs["table"] = self.ffi.DeviceBuffer(self.surf.table.nbytes).upload(self.surf.table)
        return self.bufs["table"]

    def free(self):
        for d in self.bufs.values():
            d.free()
        if self.surf is not None:
            self.surf.free()
        if self.car is not None:
            self.car.free()


def image_of(raw, nv12, bw, bh, pitch):
    """One device image (flat bytes, rows of `pitch` pixels) -> dense BGR [bh, bw, 3] or NV12 [bh * 3 // 2, bw]."""
    return raw.reshape(bh * 3 // 2, pitch)[:, :bw] if nv12 else raw.reshape(bh, pitch, 3)[:, :bw]


def plane_of(raw, dtype, bw, bh, pitch):
    """One device image of one channel (flat bytes, rows of `pitch` pixels of `dtype`) -> dense [bh, bw] of that type."""
    return raw.view(dtype).reshape(bh, pitch)[:, :bw]


def check_plane(got, want, fixed, what, under=0):
    """One one-channel image [BH, BW] (uint8 or uint16) against the yardstick's at tolerance 0.  fixed: the pixels whose value no frame
    decides (a remapper's footprints outside the frame, a stitch's pixels no camera covers), asserted on their own first: `under` there
    -- 0, or an image [BH, BW] (the car sprite)."""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, want %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got[fixed] != (under[fixed] if isinstance(under, np.ndarray) else under)
    assert not bad.any(), "%s: %d pixels that no frame reaches are not %s (first at %s: %d)" % (
        what, int(bad.sum()), "the car" if isinstance(under, np.ndarray) else "0", np.argwhere(fixed)[np.argmax(bad)].tolist(), int(got[fixed][bad][0]))
    if not np.array_equal(got, want):
        raise AssertionError("%s: %d of %d pixels differ; %s" % (what, int((got != want).sum()), got.size, first_difference(got, want)))


def run_batches(ffi, launch, sync, image_bytes, nv12, bw, bh, pitch, batches, want, what, balance=False, nb_env=0, black=False, plane=None,
                under=0):
    """launch(B, d_out) enqueues a step over the first B frame sets into d_out; every image of every batch against want = (bgr, nv12, none),
    the sentinel fill before and the guard image after each run.  plane: np.uint8 / np.uint16 -- the images are one-channel planes of that
    type, want = (images [n, bh, bw], None, the pixels no frame reaches) and every image goes through check_plane(..., under)."""
    want_bgr, want_nv12, none = want
    d_out = ffi.DeviceBuffer((max(batches) + 1) * image_bytes)
    try:
        for B in batches:
            d_out.fill(FILL)
            launch(B, d_out)
            sync()
            raw = d_out.download((B + 1, image_bytes))
            assert (raw[B] == FILL).all(), "%s, batch %d: %d bytes of the guard image behind image %d were written (first at byte %d)" % (
                what, B, int((raw[B] != FILL).sum()), B - 1, int(np.argmax(raw[B] != FILL)))
            for b in range(B):
                if plane is not None:
                    check_plane(plane_of(raw[b], plane, bw, bh, pitch), want_bgr[b], none, "%s, %s" % (what, where(B, b, balance, nb_env)), under)
                    continue
                check_image(image_of(raw[b], nv12, bw, bh, pitch), want_bgr[b], none, "%s, %s" % (what, where(B, b, balance, nb_env)),
                            "nv12" if nv12 else "bgr", black, want_nv12=want_nv12[b] if nv12 else None)
    finally:
        d_out.free()


def stitch_handle(ffi, SB, inputs, want, inp, out, blend, balance, batches=BATCHES, cfg=SMALL_CFG, nb_env=0, host_entry=True, one_slice=False, **kw):
    """One BevGenerator over `batches` through the device-resident entry, then (packed handles) the host entry on 17 sets in reversed order.
    inp: 'bgr', 'nv12', 'surfaces', or 'yuyv' / 'uyvy' where `inputs` has those forms.  one_slice: a balance handle that does not cut its
    step into slices (the plan's padded scratch), for the position a failure names."""
    fw = cfg["FRAME_WIDTH"]
    what = "%s -> %s, blend %d balance %d" % (inp, out, blend, balance)
    kw = dict(dict(blend=blend, balance=balance, input_format=inp if inp in ("bgr",) + tuple(inputs.yuv422) else "nv12", output_format=out), **kw)
    if inp == "surfaces":
        kw["input_pitch"] = fw + 4
    bev = generator(SB, small_rig(), cfg, **kw)
    info = bev.plan_info()
    assert info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0, what   # the unit kernels run
    car = inputs.car.ptr
    if inp == "surfaces":
        d_table = inputs.table()
        launch = lambda B, d_out: bev.run_surface_table(d_table.ptr, B, car, d_out.ptr, out_bytes=d_out.nbytes)
    else:
        d_in = inputs.packed(inp)
        assert bev.in_set_bytes * inputs.nv.shape[0] == d_in.nbytes
        launch = lambda B, d_out: bev.run_device(d_in.ptr, B, car, d_out.ptr, out_bytes=d_out.nbytes)
    nv12 = out == "nv12"
    run_batches(ffi, launch, bev.sync, bev.out_image_bytes, nv12, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], bev.out_pitch, batches, want, what,
                balance=balance and not one_slice, nb_env=nb_env)
    if host_entry and inp != "surfaces":
        host = inputs.host(inp)
        car_host = inputs.car.download(want[0][0].shape)
        got = bev.batch(host[:17][::-1], car_host)
        for i in range(17):
            check_image(got[i], want[0][16 - i], want[2], "%s, host entry, reversed: position %d = set %d; %s" % (
                what, i, 16 - i, where(17, i, balance and not one_slice, nb_env)), out, want_nv12=want[1][16 - i] if nv12 else None)
    return bev


# ---------------------------------------------------------------------------------------------------------------
# worker processes (tests/_*_worker.py): the library reads its BEVW_* switches once per process
# ---------------------------------------------------------------------------------------------------------------
DEAD_STATUS = (134, 139, 124, 137)   # abort, segmentation fault, and the two statuses of a time limit


def run_child(worker, args, set_env=None, drop_env=(), timeout=180, expect="worker OK"):
    """Runs tests/<worker> (or an absolute path) in a fresh process and returns it.  drop_env: names or prefixes removed from the
    environment first, set_env: the switches set then; timeout in seconds; expect: the stdout line that proves success.  A child that
    exits non-zero or without that line fails the test; one that died (time limit, signal, DEAD_STATUS) ends the pytest session."""
    name = os.path.basename(worker)
    env = {k: v for k, v in os.environ.items() if not k.startswith(tuple(drop_env))}
    env.update(set_env or {})
    cmd = [sys.executable, os.path.join(ROOT, "tests", worker)] + [str(a) for a in args]
    try:
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        print(e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace"))
        pytest.exit("%s %s ran into its time limit of %s s: nothing more may start on this GPU" % (name, set_env or "", timeout))
    print(p.stdout)
    tails = "%s\n%s" % (p.stdout[-4000:], p.stderr[-4000:])
    if p.returncode < 0 or p.returncode in DEAD_STATUS:
        pytest.exit("%s %s died with status %d: nothing more may start on this GPU\n%s" % (name, set_env or "", p.returncode, tails))
    assert p.returncode == 0, "%s %s: worker exit %d\n%s" % (name, set_env or "", p.returncode, tails)
    assert expect in p.stdout, "%s %s: no '%s' line\n%s" % (name, set_env or "", expect, tails)
    return p


def worker_library(switches, only=()):
    """The first call of a worker's main(): asserts that `switches` ({NAME: value}) are in the environment -- the library reads them when it
    loads -- and that no other variable with a prefix in `only` is; then loads the library.  -> (ffi, SB)."""
    for k, v in switches.items():
        assert os.environ.get(k) == v, "%s=%s must be set before the library loads" % (k, v)
    assert not only or sorted(k for k in os.environ if k.startswith(tuple(only))) == sorted(switches), "exactly the switches of this worker"
    from cameracalibration_amd import _ffi
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV

    _ffi.require_device()
    return _ffi, surroundBEV
