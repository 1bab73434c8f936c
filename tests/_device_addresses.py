"""Caller buffers at hostile ADDRESSES for the device-resident entry points: the catalogue of tests/test_device_addresses_gpu.py (what the
kernels make of them) and tests/test_device_addresses_host.py (a census, so that no family passes emptily), and the arena both speak about.

bevw_run_device, bevw_remap_device and the two JPEG *_run_device calls carry a dispatch that depends on nothing but the caller's pointers
(csrc/bevwarp.hip: run_device's `aligned4`, remap_step; csrc/bevwarp_jpeg.hip: `aligned`; include/bevwarp.h states the contract next to
bevw_run_device): on dense handles any byte alignment of d_frames, d_car and d_out is accepted and served by the per-pixel kernels, a
pitched handle refuses it.  A step here names the byte offset of each of its buffers from a 16-byte aligned base inside an Arena and the
path it must take -- PATH_UNITS (the tile plan), PATH_PER_PIXEL, or REFUSE -- by that rule and nothing else: an offset off a 4-byte
boundary, or a per-pixel schedule, is the only thing that keeps a step of these handles away from the units.

Shape: SMALL_CFG (320 x 256 -> 248 x 250), small_rig(), batch 3, graded frame sets (tests/_balance_content.graded: brightness differs per
camera and per set, so the luminance deltas of the three sets differ) and a random car.  The other pixel formats are derived from the BGR
sets (input generation only); the expected images are the oracle's on the spec-converted frames, as everywhere else in the suite."""
import collections
import functools

import numpy as np

from tests import _balance_content as BC
from tests import _jpeg_common as JC
from tests import _nv12_spec as S
from tests import _yuv422_spec as Y
from tests._harness import FILL, SMALL_CFG, random_car

BATCH = 3
SEED = 1600
SLACK = 16                                                                  # bytes of an arena in front of and behind the payload's base
MODES = collections.OrderedDict([("direct", (False, False)), ("blend", (True, False)), ("balance", (True, True))])   # (blend, balance)
CFGS = {"small": SMALL_CFG, "bw250": dict(SMALL_CFG, BEV_WIDTH=250)}       # bw250: the plan's padded scratch and k_plan_unpad
UNITS, PER_PIXEL, REFUSE = "units", "per_pixel", "refuse"
ODD = (1, 2, 3)
ZERO = dict(frames=0, car=0, out=0)


# ---------------------------------------------------------------------------------------------------------------
# the arena
# ---------------------------------------------------------------------------------------------------------------
class Arena:
    """A device buffer of SLACK + nbytes + SLACK bytes.  place(payload, off) fills ALL of it with 0x5A and uploads the payload at base + off,
    clear(off) only fills; both return the device address base + off (base = the allocation + SLACK, 16-byte aligned).  read(off, n) returns
    the n payload bytes after asserting that every byte in front of base + off and behind base + off + n still holds the fill."""

    def __init__(self, ffi, nbytes):
        self.nbytes, self.buf = int(nbytes), ffi.DeviceBuffer(int(nbytes) + 2 * SLACK)
        assert self.buf.ptr % 16 == 0, "the allocator's alignment: offsets would not be what they say"

    def clear(self, off=0):
        assert 0 <= off < SLACK
        self.buf.fill(FILL)
        return self.buf.ptr + SLACK + off

    def place(self, payload, off=0):
        payload = np.ascontiguousarray(payload)
        assert payload.nbytes <= self.nbytes
        p = self.clear(off)
        self.buf.upload(payload, offset=SLACK + off)
        return p

    def read(self, off, n, what):
        raw = self.buf.download((self.buf.nbytes,))
        lo, hi = SLACK + off, SLACK + off + n
        front, behind = raw[:lo] != FILL, raw[hi:] != FILL
        assert not front.any(), "%s: %d bytes in front of the buffer were written (the nearest %d bytes before it)" % (
            what, int(front.sum()), lo - int(np.flatnonzero(front)[-1]))
        assert not behind.any(), "%s: %d bytes behind the last image were written (the first %d bytes after it)" % (
            what, int(behind.sum()), int(np.flatnonzero(behind)[0]))
        return raw[lo:hi]

    def untouched(self, what):
        raw = self.buf.download((self.buf.nbytes,))
        assert (raw == FILL).all(), "%s: %d bytes of the output arena were written by a refused step" % (what, int((raw != FILL).sum()))

    def free(self):
        self.buf.free()


# ---------------------------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def content(fmt):
    """(BATCH frame sets in pixel format `fmt` as the engine takes them, the BGR frame sets the input specification makes of them)."""
    fw, fh = SMALL_CFG["FRAME_WIDTH"], SMALL_CFG["FRAME_HEIGHT"]
    bgr = BC.graded(np.random.default_rng(SEED), BATCH, fw, fh)
    if fmt == "bgr":
        native = back = bgr
    elif fmt == "nv12":
        native = np.stack([S.bgr_to_nv12(s) for s in bgr])
        back = np.stack([S.nv12_to_bgr(s) for s in native])
    else:
        native = np.stack([Y.bgr_to_yuv422(s, fmt) for s in bgr])
        back = np.stack([Y.yuv422_to_bgr(s, fmt) for s in native])
    for a in (native, back):
        a.setflags(write=False)
    return native, back


@functools.lru_cache(maxsize=None)
def car(cfg_name):
    c = random_car(np.random.default_rng([SEED, sorted(CFGS).index(cfg_name)]), CFGS[cfg_name])
    c.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------------------------
# the stitch handle
# ---------------------------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "name frames car out expect")
Handle = collections.namedtuple("Handle", "name family cfg inp out mode schedule pitch surfaces with_car steps")


def _expect(offs, per_pixel=False, pitched=False):
    odd = any(v % 4 for v in offs.values())
    return REFUSE if (pitched and odd) else PER_PIXEL if (odd or per_pixel) else UNITS


def _steps(prefix, moves, per_pixel=False, pitched=False):
    """The aligned control, every move, the aligned control AGAIN: the handle must come back to the path it had."""
    out = []
    for label, offs in [("control before", {})] + [(" ".join("%s+%d" % kv for kv in sorted(m.items())), m) for m in moves] + [("control after", {})]:
        o = dict(ZERO, **offs)
        out.append(Step("%s, %s" % (prefix, label), o["frames"], o["car"], o["out"], _expect(o, per_pixel, pitched)))
    return tuple(out)


def _handle(family, cfg, inp, out, mode, moves, schedule="plan", pitch="dense", surfaces=False, with_car=True):
    name = "%s: %s%s -> %s, %s" % (family, "surfaces " if surfaces else "", inp, out, mode)
    return Handle(name, family, cfg, inp, out, mode, schedule, pitch, surfaces, with_car,
                  _steps(name, moves, per_pixel=schedule == "per_pixel", pitched=pitch == "aligned"))


def stitch_handles():
    hs = []
    for mode in MODES:
        hs.append(_handle("bgr", "small", "bgr", "bgr", mode, [{w: o} for w in ("frames", "car", "out") for o in ODD]))
        for inp in ("nv12", "yuyv", "uyvy"):   # +4, +8, +12: the units; a balance step's 4:2:2 V sums then leave their 16-byte loads
            hs.append(_handle("formats_in", "small", inp, "bgr", mode, [{"frames": o} for o in ODD + (4, 8, 12)]))
        hs.append(_handle("nv12_out", "small", "bgr", "nv12", mode,
                          [{"out": o} for o in ODD] + [{"car": o} for o in ODD] + [{"out": 1, "car": 3}, {"out": 2, "car": 2}, {"out": 3, "car": 1}]))
        hs.append(_handle("padded_scratch", "bw250", "bgr", "bgr", mode, [{"out": o} for o in ODD] + [{"car": 2}]))
        hs.append(_handle("no_car", "small", "bgr", "bgr", mode, [{"frames": 1}, {"out": 3}], with_car=False))
        hs.append(_handle("per_pixel_schedule", "small", "bgr", "bgr", mode, [{"frames": 1}, {"out": 1}, {"car": 1}], schedule="per_pixel"))
        hs.append(_handle("surfaces", "small", "nv12", "bgr", mode, [{"out": o} for o in ODD] + [{"car": 2}], surfaces=True))
        hs.append(_handle("pitched", "small", "bgr", "bgr", mode, [{"frames": 1}, {"car": 1}, {"out": 1}], pitch="aligned"))
    return hs


# ---------------------------------------------------------------------------------------------------------------
# the three-channel remapper
# ---------------------------------------------------------------------------------------------------------------
REMAP_MAPS = ("undistort_front", "stripes")     # the fisheye undistort maps of small_rig()'s front camera; a folded family of tests/_caller_maps.py
REMAP_INPUTS, REMAP_OUTPUTS = ("bgr", "nv12", "yuyv"), ("bgr", "nv12")
RStep = collections.namedtuple("RStep", "name src dst expect")
RHandle = collections.namedtuple("RHandle", "name maps inp out steps")


def remap_handles():
    hs = []
    for maps in REMAP_MAPS:
        for inp in REMAP_INPUTS:
            for out in REMAP_OUTPUTS:
                name = "remap %s: %s -> %s" % (maps, inp, out)
                moves = [("control before", 0, 0)] + [("src+%d" % o, o, 0) for o in ODD] + [("dst+%d" % o, 0, o) for o in ODD] + [
                    ("src+4", 4, 0), ("src+12", 12, 0), ("control after", 0, 0)]
                hs.append(RHandle(name, maps, inp, out, tuple(RStep("%s, %s" % (name, l), s, d, PER_PIXEL if (s % 4 or d % 4) else UNITS)
                                                              for l, s, d in moves)))
    return hs


@functools.lru_cache(maxsize=None)
def remap_frames(sw, sh, inp):
    """BATCH random frames of sw x sh texels in format `inp`, and the BGR frames the input specification makes of them."""
    rng = np.random.default_rng([SEED, sw, sh, REMAP_INPUTS.index(inp)])
    if inp == "bgr":
        raw = rng.integers(0, 256, (BATCH, sh, sw, 3), dtype=np.uint8)
        return raw, raw
    if inp == "nv12":
        raw = S.random_nv12(rng, (BATCH,), sw, sh)
        return raw, S.nv12_to_bgr(raw)
    raw = Y.random_yuv422(rng, (BATCH,), sw, sh)
    return raw, Y.yuv422_to_bgr(raw, inp)


# ---------------------------------------------------------------------------------------------------------------
# JPEG
# ---------------------------------------------------------------------------------------------------------------
JPEG_SIZES = ((40, 56), (17, 33), (100, 75))                 # (h, w), of tests/_jpeg_common.SIZES
JPEG_FILES = 3                                               # files per decode, images per encode: kinds 0, 1, 2 of _jpeg_common.image
JPEG_SUBSAMPLINGS = (("420", 2), ("444", 0))                 # name, Pillow's code
DECODE_OFFSETS, DECODE_PITCH_EXTRA, DECODE_STRIDE_EXTRA = (0, 1, 2, 3), (0, 1, 4, 7), (0, 5)
ENCODE_OFFSETS, ENCODE_PITCH_EXTRA, ENCODE_STRIDE_EXTRA = ODD, (1, 4), (0, 5)
ENCODE_PADDING = 77
JCase = collections.namedtuple("JCase", "name h w off pitch stride")


def decode_cases(h, w, sub):
    return [JCase("jpeg decode %dx%d %s, d_out+%d pitch w*3+%d stride pitch*h+%d" % (w, h, sub, off, pe, se), h, w, off, w * 3 + pe, (w * 3 + pe) * h + se)
            for off in DECODE_OFFSETS for pe in DECODE_PITCH_EXTRA for se in DECODE_STRIDE_EXTRA]


def encode_cases(h, w):
    return [JCase("jpeg encode %dx%d, d_bgr+%d pitch w*3+%d stride pitch*h+%d" % (w, h, off, pe, se), h, w, off, w * 3 + pe, (w * 3 + pe) * h + se)
            for off in ENCODE_OFFSETS for pe in ENCODE_PITCH_EXTRA for se in ENCODE_STRIDE_EXTRA]


def jpeg_images(h, w):
    return np.stack([JC.image(h, w, kind) for kind in range(JPEG_FILES)])


# ---------------------------------------------------------------------------------------------------------------
# the census (tests/test_device_addresses_host.py): what the issue of this catalogue names, family by family
# ---------------------------------------------------------------------------------------------------------------
def moved(step):
    """{(buffer, offset)} of a stitch step's buffers that are off their base."""
    return {(w, getattr(step, w)) for w in ("frames", "car", "out") if getattr(step, w)}


REQUIRED = {   # family -> the (buffer, offset) moves every mode of it must hold, each on a step of its own unless marked
    "bgr": {(w, o) for w in ("frames", "car", "out") for o in ODD},
    "formats_in": {("frames", o) for o in ODD + (4, 8, 12)},
    "nv12_out": {(w, o) for w in ("car", "out") for o in ODD},
    "padded_scratch": {("out", 1), ("out", 2), ("out", 3), ("car", 2)},
    "no_car": {("frames", 1), ("out", 3)},
    "per_pixel_schedule": {("frames", 1), ("out", 1), ("car", 1)},
    "surfaces": {("out", 1), ("out", 2), ("out", 3), ("car", 2)},
    "pitched": {("frames", 1), ("car", 1), ("out", 1)},
}
FAMILY_INPUTS = {"formats_in": ("nv12", "yuyv", "uyvy")}   # families that must come in more than one input format


def all_names():
    names = [s.name for h in stitch_handles() for s in h.steps] + [s.name for h in remap_handles() for s in h.steps]
    for h, w in JPEG_SIZES:
        for sub, _ in JPEG_SUBSAMPLINGS:
            names += [c.name for c in decode_cases(h, w, sub)]
        names += [c.name for c in encode_cases(h, w)]
    return names
