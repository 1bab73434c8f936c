"""Shared by tests/test_gray16_host.py and tests/test_gray16_gpu.py: 16-bit single-channel images through the remapper
(bevw_remapper_set_depth).  The expected value is always oracle.remap on the uint16 array; the frames are full-range random uint16 -- with
data below 2^14 the exact-integer round-half-even form equals the float arithmetic everywhere (tests/test_gray16_host.py has the census),
and a test on 12-bit data could not tell the two apart."""
import numpy as np

from tests import _caller_maps as CM

CASES = [(name, size) for name in CM.FAMILIES for size in CM.sizes(name)]
CASE_IDS = ["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASES]
CENSUS_SIZE = (64, 48, 160, 120)   # sw, sh, dw, dh
CENSUS_SEEDS = (1, 2, 3)


def frames16(sw, sh, n, seed):
    """n frames of uniform random uint16 over the full range."""
    f = np.random.default_rng([int(seed), sw, sh]).integers(0, 65536, (n, sh, sw), dtype=np.uint16)
    assert f.max() >= 0xff00 and f.min() < 0x100
    return f


def want16(oracle, frames, m1, m2):
    assert frames.dtype == np.uint16
    return np.stack([oracle.remap(f, m1, m2) for f in frames])


def taps_and_weights(src, m1, m2):
    """The four taps (int64, a tap outside the frame 0) and the four integer weights w' = 1024 * w of every destination pixel."""
    sh, sw = src.shape
    sx, sy = m1[..., 0].astype(np.int64), m1[..., 1].astype(np.int64)
    code = m2.astype(np.int64) & 1023
    fx, fy = code & 31, code >> 5
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = sx + dx, sy + dy
            ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
            taps.append(np.where(ok, src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64), 0))
    return taps, [(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx]


def exact_half_even(src, m1, m2):
    """The exact-integer form round-half-even((sum t w') / 1024): what the float arithmetic would give if its products did not round."""
    t, w = taps_and_weights(src, m1, m2)
    s = sum(a * b for a, b in zip(t, w))
    q, r = s >> 10, s & 1023
    return np.clip(q + ((r > 512) | ((r == 512) & (q & 1 == 1))), 0, 65535).astype(np.uint16)


def half_up(src, m1, m2):
    """The fixed-point form of the 8-bit path carried over: (sum t w' + 512) >> 10."""
    t, w = taps_and_weights(src, m1, m2)
    return np.clip((sum(a * b for a, b in zip(t, w)) + 512) >> 10, 0, 65535).astype(np.uint16)


def assert_same16(got, want, outside, what):
    """One uint16 image of a remapper [DH, DW]; outside: pixels whose footprint lies outside the frame, which must be 0 (asserted first)."""
    assert got.shape == want.shape and got.dtype == np.uint16 and want.dtype == np.uint16, what
    assert not got[outside].any(), "%s: a pixel whose footprint lies outside the frame is not 0" % what
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first at %s)" % (what, int((got != want).sum()), got.size,
                                                                                    tuple(int(i) for i in np.argwhere(got != want)[0]))


# ---- a harness Remapper (tests/_harness.py) at 16 bits: the depth through ctypes, uint16 in and out ----
def set_depth(rem, bits):
    rem.ffi.check(rem.L.bevw_remapper_set_depth(rem.r, bits))
    assert rem.L.bevw_remapper_depth(rem.r) == bits


def remap16(rem, frames):
    """Host uint16 frames [n, sh, sw] -> host uint16 images over a 0x5a5a fill (bevw_remap on a 16-bit remapper)."""
    assert frames.dtype == np.uint16
    dw, dh = rem.size[2:]
    got = np.full((frames.shape[0], dh, dw), 0x5a5a, np.uint16)
    rem.ffi.check(rem.L.bevw_remap(rem.r, rem.ffi.ptr(np.ascontiguousarray(frames)), frames.shape[0], rem.ffi.ptr(got)))
    return got


GUARD = 64   # bytes of 0x5a on either side of a device buffer under test


class Guarded:
    """A device buffer of exactly `nbytes` between two GUARD-byte runs of 0x5a, at byte offset `shift` from a 4-byte boundary."""

    def __init__(self, ffi, nbytes, shift=0):
        self.nbytes, self.shift = int(nbytes), int(shift)
        self.buf = ffi.DeviceBuffer(2 * GUARD + self.nbytes + 8)
        self.buf.fill(0x5a)
        self.ptr = self.buf.ptr + GUARD + self.shift

    def upload(self, a):
        assert a.nbytes == self.nbytes
        self.buf.upload(np.ascontiguousarray(a), offset=GUARD + self.shift)
        return self

    def download(self, shape, dtype=np.uint16):
        raw = self.buf.download((2 * GUARD + self.nbytes + 8,))
        lo, hi = raw[:GUARD + self.shift], raw[GUARD + self.shift + self.nbytes:]
        assert (lo == 0x5a).all() and (hi == 0x5a).all(), "a guard byte was written"
        return raw[GUARD + self.shift:GUARD + self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.download((2 * GUARD + self.nbytes + 8,)) == 0x5a).all())

    def free(self):
        self.buf.free()
