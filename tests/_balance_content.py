"""Frame sets with distinct brightness and colour cast per set, for the balance chain (balance=True): the pool of
tests/test_balance_content_host.py (its preconditions, no GPU) and tests/test_balance_content_gpu.py.

The balance modes are the only arithmetic of the engine that depends on statistics of the frames: per-frame V sums -> fp64 means ->
rounded per-camera deltas -> the HSV round trip with a saturating V -> per-image channel sums -> fp64 gains -> saturation.  Every one
of them is stored per frame set and indexed on the host and in the kernels; uniform random frames give every set of a batch the same
statistics (delta 0, gains within 1e-3 of 1), so an index that is wrong by a set, a camera or a ring slot changes nothing there.

The pool: N = 33 frame sets for tests/_harness.SMALL_CFG (33 is a key of PLAIN / SLICES in tests/_harness.py: a
balance step of 33 runs as two slices of 16 and 17 frame sets).  GRADED sets are uniform random bytes times a factor per (set, camera,
channel) drawn from 8 .. 256, then >> 8: brightness differs per camera and per set, the cast per set.  SPECIAL sets sit at fixed
positions, five of them in the first nine (batch 9, and the reversed host entry over the first 17):

   0 black       all four frames 0: deltas 0, channel sums 0, gains 0 / 0
   1 white       all four frames 255
   3 black_white cameras 0, 2, 3 black and camera 1 white, each with one 12 x 12 grey patch (250 in the black frames, 100 in the white
                 one: 0.44 and 0.27 of a mean): deltas +64 and -191, the patches saturate at V = 255 and V = 0
   5 dead        B is 0 in every texel and no texel is black: the B sum of the pre-gain image is 0, its gain inf beside two finite ones
   7 tie         grey stripes: camera c has level a left and b in its last n columns, TIE_LEVELS.  The V means are 125.2, 128.2, 128.2,
                 129.2, their mean 127.7: vmean - m is -0.5 (k = -1, odd) and -1.5 (k = -2, even) EXACTLY in fp64 for cameras 1, 2, 3,
                 so half-even gives (2, 0, 0, -2), floor(x + 0.5) gives (2, 0, 0, -1) and half away from zero (2, -1, -1, -2).  The
                 means straddle 128, where the fp64 grid changes: (s0 + s1 + s2 + s3) / (4 npx) is one ulp above the mean of the four
                 means, which moves camera 3 off its tie and rounds it to -1
  16 dark        bytes 0 .. 3 (the first set of the second slice of a balance step of 33)
  20 near_dead   as `dead`, but some 8 x 8 cells have B = 1: the B gain exceeds 255 and is finite

Constant regions of the special sets are 2 x 2-aligned and their colours are fixed points of BGR -> YUV -> BGR (fixed_colours), so
the NV12 / YUYV / UYVY forms of a special set convert back to the BGR set itself; the graded sets do not (limited range, shared
chroma), which is why the preconditions are asserted per pixel format.  The other formats are derived through
_nv12_spec.bgr_to_nv12 / _yuv422_spec.bgr_to_yuv422 (input generation only); expected images are always the oracle's on the
spec-converted frames (_nv12_spec.nv12_to_bgr, _yuv422_spec.yuv422_to_bgr), as in the NV12 and 4:2:2 modules.

Chain restates RefBevGenerator(balance=True) from the oracle's own steps, so that single quantities can be swapped between frame sets
(the mutants of the host module)."""
import functools
import math

import numpy as np

from tests import _nv12_spec as S
from tests import _yuv422_spec as Y
from tests._harness import SMALL_CFG as CFG, random_car, small_rig, uncovered  # noqa: F401

N = 33
SEED = 7100
FORMATS = ("bgr", "nv12", "yuyv", "uyvy")
SPECIAL = {0: "black", 1: "white", 3: "black_white", 5: "dead", 7: "tie", 16: "dark", 20: "near_dead"}
AT = {name: b for b, name in SPECIAL.items()}
GRADED = tuple(b for b in range(N) if b not in SPECIAL)
WHITE_CAMERA = 1
TIE_LEVELS = ((118, 130, 192), (81, 140, 256), (123, 136, 128), (128, 134, 64))   # per camera: level, level of the last n columns, n
TIE_DELTAS = {"even": (2, 0, 0, -2), "floor": (2, 0, 0, -1), "away": (2, -1, -1, -2), "sums": (2, 0, 0, -1)}
SLICE_FIRST = (0, 16)   # the first frame sets of the two slices of a balance step of 33


def slice_first(b):
    return SLICE_FIRST[1] if b >= SLICE_FIRST[1] else SLICE_FIRST[0]


# ---------------------------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------------------------
def graded(rng, n, fw, fh):
    """n graded frame sets [n, 4, fh, fw, 3]: uniform random bytes times a factor per (set, camera, channel) of 8 .. 256, >> 8."""
    raw = rng.integers(0, 256, (n, 4, fh, fw, 3), dtype=np.uint8).astype(np.uint16)
    factor = rng.integers(8, 257, (n, 4, 1, 1, 3)).astype(np.uint16)
    return ((raw * factor) >> 8).astype(np.uint8)


def round_trip(colours):
    """Constant colours [n, 3] through bgr_to_nv12 / nv12_to_bgr and bgr_to_yuv422 / yuv422_to_bgr (the two agree on constant regions)."""
    img = np.repeat(np.repeat(np.asarray(colours, np.uint8)[:, None, None, :], 2, 1), 2, 2)
    a = S.nv12_to_bgr(S.bgr_to_nv12(img))[:, 0, 0]
    b = Y.yuv422_to_bgr(Y.bgr_to_yuv422(img, "yuyv"), "yuyv")[:, 0, 0]
    assert np.array_equal(a, b)
    return a


@functools.lru_cache(maxsize=None)
def fixed_colours(blue):
    """Colours (blue, G, R) with max(G, R) >= 32 that BGR -> YUV -> BGR returns unchanged, as an array [n, 3]."""
    g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    c = np.stack([np.full(g.size, blue), g.ravel(), r.ravel()], -1).astype(np.uint8)
    c = c[np.maximum(c[:, 1], c[:, 2]) >= 32]
    return c[(round_trip(c) == c).all(1)]


def mosaic(rng, colours, fw, fh, cell=8):
    """Four frames [4, fh, fw, 3] of cell x cell squares, each of a colour drawn from `colours`."""
    ny, nx = -(-fh // cell), -(-fw // cell)
    pick = colours[rng.integers(0, len(colours), (4, ny, nx))]
    return np.repeat(np.repeat(pick, cell, 1), cell, 2)[:, :fh, :fw]


def special(name, fw, fh, seed=SEED):
    rng = np.random.default_rng([seed, sorted(AT).index(name)])
    f = np.zeros((4, fh, fw, 3), np.uint8)
    if name == "white":
        f[:] = 255
    elif name == "black_white":
        f[WHITE_CAMERA] = 255
        y0, x0 = fh // 2 - 6, fw // 2 - 6
        for c in range(4):
            f[c, y0:y0 + 12, x0:x0 + 12] = 100 if c == WHITE_CAMERA else 250
    elif name == "dead":
        f = mosaic(rng, fixed_colours(0), fw, fh)
    elif name == "near_dead":
        f = mosaic(rng, fixed_colours(0), fw, fh).copy()
        ones = fixed_colours(1)
        for c in range(4):
            for _ in range(24):
                y, x = 8 * int(rng.integers(0, fh // 8)), 8 * int(rng.integers(0, fw // 8))
                f[c, y:y + 8, x:x + 8] = ones[rng.integers(0, len(ones))]
    elif name == "tie":
        assert (fw, fh) == (320, 256), "the tie levels are worked out for 320 x 256 frames"
        for c, (a, b, n) in enumerate(TIE_LEVELS):
            f[c], f[c, :, fw - n:] = a, b
    elif name == "dark":
        f = rng.integers(0, 4, (4, fh, fw, 3), dtype=np.uint8)
    else:
        assert name == "black", name
    return f


@functools.lru_cache(maxsize=None)
def bgr_pool(seed=SEED):
    """The pool as BGR frames [N, 4, FH, FW, 3] (read-only)."""
    fw, fh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]
    pool = graded(np.random.default_rng(seed), N, fw, fh)
    for b, name in SPECIAL.items():
        pool[b] = special(name, fw, fh, seed)
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def forms(fmt, seed=SEED):
    """(the pool in pixel format `fmt` as the engine takes it, the BGR frames the input specification makes of it), both read-only."""
    bgr = bgr_pool(seed)
    if fmt == "bgr":
        return bgr, bgr
    if fmt == "nv12":
        native = np.stack([S.bgr_to_nv12(s) for s in bgr])
        back = np.stack([S.nv12_to_bgr(s) for s in native])
    else:
        native = np.stack([Y.bgr_to_yuv422(s, fmt) for s in bgr])
        back = np.stack([Y.yuv422_to_bgr(s, fmt) for s in native])
    native.setflags(write=False)
    back.setflags(write=False)
    return native, back


def car(cfg=CFG, seed=SEED):
    return random_car(np.random.default_rng([seed, 99]), cfg)


# ---------------------------------------------------------------------------------------------------------------
# the balance chain from the oracle's own steps
# ---------------------------------------------------------------------------------------------------------------
class Chain:
    """RefBevGenerator(balance=True) restated: sum_v -> orc_round_delta -> orc_luminance_shift -> RefBevGenerator(balance=False) ->
    orc_channel_sums -> orc_gain -> add_sat with the car.  `mean` and `rounding` select the two arithmetic mutants."""

    def __init__(self, oracle, blend, cfg=CFG, rig=None):
        self.O, self.L = oracle, oracle.lib()
        self.plain = oracle.RefBevGenerator(rig or small_rig(), cfg, blend=blend, balance=False)

    def vsums(self, frames4):
        return [self.O.sum_v(f) for f in frames4]

    def raw_deltas(self, frames4, mean="means"):
        """vmean - m per camera, in fp64 as the oracle computes it ('means') or from the mean of the four sums ('sums')."""
        npx = frames4[0].size // 3
        s = self.vsums(frames4)
        m = [v / npx for v in s]
        vmean = (m[0] + m[1] + m[2] + m[3]) / 4 if mean == "means" else (s[0] + s[1] + s[2] + s[3]) / (4 * npx)
        return [vmean - x for x in m]

    def deltas(self, frames4, mean="means", rounding="even"):
        raw = self.raw_deltas(frames4, mean)
        if rounding == "even":
            return tuple(int(self.L.orc_round_delta(x)) for x in raw)
        if rounding == "floor":
            return tuple(int(math.floor(x + 0.5)) for x in raw)
        assert rounding == "away"
        return tuple(int(math.copysign(math.floor(abs(x) + 0.5), x)) for x in raw)

    def shift(self, frame, delta):
        f = np.ascontiguousarray(frame, np.uint8)
        out = np.empty_like(f)
        self.L.orc_luminance_shift(f.ctypes.data, f.size // 3, int(delta), out.ctypes.data)
        return out

    def pregain(self, frames4, deltas):
        """The stitched image before the colour balance, without the car."""
        return self.plain(*[self.shift(f, d) for f, d in zip(frames4, deltas)])

    def gains(self, pre):
        npx = pre.size // 3
        sums = np.zeros(3, np.uint64)
        self.L.orc_channel_sums(pre.ctypes.data, npx, sums.ctypes.data)
        B, G, R = (float(s) / npx for s in sums)
        K = (R + G + B) / 3
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.array([np.float64(K) / np.float64(B), np.float64(K) / np.float64(G), np.float64(K) / np.float64(R)], np.float64)

    def finish(self, pre, gains, car_img=None):
        img = np.ascontiguousarray(pre, np.uint8).copy()
        g = np.ascontiguousarray(gains, np.float64)
        self.L.orc_gain(img.ctypes.data, img.size // 3, g.ctypes.data)
        return self.O.add_sat(img, car_img) if car_img is not None else img
