"""Shared by tests/test_nearest_host.py, tests/test_nearest_gpu.py and tests/_nearest_worker.py: nearest-neighbour remapping of one-channel
images (bevw_remapper_set_interpolation).  The yardstick is want_nn below: the NumPy statement of cv2.remap(src, map1, map2,
cv2.INTER_NEAREST) with map1 CV_16SC2, a non-empty map2 CV_16UC1 and BORDER_CONSTANT 0 -- OpenCV's RemapInvoker adds NNDeltaTab_i[map2 & 1023]
= {fx >= 16, fy >= 16} to map1 INTO A SHORT buffer and remapNearest bounds-checks with unsigned compares.  Like the NV12 conversions it is
not pinned against a real cv2 here (there is none on our machines): tests/golden/make_nearest_goldens_with_cv2.py writes the vectors that
tests/test_nearest_cv2_probe.py would hold it to."""
import numpy as np

from tests import _caller_maps as CM

CASES = [(name, size) for name in CM.FAMILIES for size in CM.sizes(name)]
CASE_IDS = ["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASES]
LABELS = {8: (0, 7, 200, 255), 16: (0, 7, 40000, 65535)}
DTYPE = {8: np.uint8, 16: np.uint16}
WRAP_SIZES = ((32772, 4, 8, 4), (4, 32772, 8, 4))   # sw, sh, dw, dh: the only sources on which the short's wrap shows


def deltas(m2):
    a = m2.astype(np.int64) & 1023
    return ((a & 31) >= 16).astype(np.int64), ((a >> 5) >= 16).astype(np.int64)


def nearest_xy(m1, m2, wrap=True):
    """The texel cv2 picks: map1 + delta stored into a short (wrap=False: what the sum would be in an int)."""
    dx, dy = deltas(m2)
    x, y = m1[..., 0].astype(np.int64) + dx, m1[..., 1].astype(np.int64) + dy
    if wrap:
        x, y = (x + 32768) % 65536 - 32768, (y + 32768) % 65536 - 32768
    return x, y


def inside_nn(m1, m2, sw, sh, wrap=True):
    x, y = nearest_xy(m1, m2, wrap)
    return (x >= 0) & (x < sw) & (y >= 0) & (y < sh)


def want_nn(frames, m1, m2, wrap=True):
    """frames [n, sh, sw] (or one [sh, sw]) uint8 / uint16 -> the nearest remap [n, dh, dw] (or [dh, dw]) of the same dtype."""
    sh, sw = frames.shape[-2:]
    x, y = nearest_xy(m1, m2, wrap)
    ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
    picked = frames[..., np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
    return np.where(ok, picked, 0).astype(frames.dtype)


def footprint_inside(m1, sw, sh):
    """All four texels of the bilinear footprint lie inside the frame."""
    sx, sy = m1[..., 0].astype(np.int64), m1[..., 1].astype(np.int64)
    return (sx >= 0) & (sx + 1 < sw) & (sy >= 0) & (sy + 1 < sh)


def label_frames(sw, sh, n, seed, depth):
    """n frames whose texels are drawn from LABELS[depth]: class IDs, where a blend of two is the ID of nobody."""
    rng = np.random.default_rng([int(seed), sw, sh, depth])
    return np.asarray(LABELS[depth], DTYPE[depth])[rng.integers(0, 4, (n, sh, sw))]


def random_frames(sw, sh, n, seed, depth):
    """n frames of uniform random texels over the full range."""
    return np.random.default_rng([int(seed), sw, sh, depth, 1]).integers(0, 1 << depth, (n, sh, sw), dtype=DTYPE[depth])


def wrap_case(size):
    """A source of 32772 texels along one axis and map1 = 32767 on it with fx (fy) of 15 and 16 in alternate columns: the delta of 1
    makes 32768 in an int -- a texel of the frame -- and -32768 in cv2's short: 0.  -> m1, m2."""
    sw, sh, dw, dh = size
    along_x = sw > sh
    y, x = np.mgrid[0:dh, 0:dw]
    f = np.where(x % 2 == 1, 16, 15)
    m1 = np.stack([np.full((dh, dw), 32767) if along_x else x % sw, y % sh if along_x else np.full((dh, dw), 32767)], -1).astype(np.int16)
    m2 = (f if along_x else f << 5).astype(np.uint16)
    return np.ascontiguousarray(m1), np.ascontiguousarray(m2)


def assert_same_nn(got, want, outside, what):
    """One image of a remapper [DH, DW]; outside: pixels whose nearest texel lies outside the frame, which must be 0 (asserted first)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    assert not got[outside].any(), "%s: a pixel whose nearest texel lies outside the frame is not 0" % what
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first at %s)" % (what, int((got != want).sum()), got.size,
                                                                                    tuple(int(i) for i in np.argwhere(got != want)[0]))


def assert_batch_nn(got, want, outside, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for b in range(got.shape[0]):
        assert_same_nn(got[b], want[b], outside, "%s, image %d" % (what, b))


def assert_labels(got, depth, what):
    assert np.isin(got, LABELS[depth]).all(), "%s: a value outside the label set" % what


# ---- a harness Remapper (tests/_harness.py) in nearest mode: the setters through ctypes, either depth in and out ----
def set_interpolation(rem, nearest):
    v = rem.ffi.INTER_NEAREST if nearest else rem.ffi.INTER_LINEAR
    rem.ffi.check(rem.L.bevw_remapper_set_interpolation(rem.r, v))
    assert rem.L.bevw_remapper_interpolation(rem.r) == v


def set_depth(rem, bits):
    rem.ffi.check(rem.L.bevw_remapper_set_depth(rem.r, bits))
    assert rem.L.bevw_remapper_depth(rem.r) == bits


def remap_nn(rem, frames):
    """Host frames [n, sh, sw] -> host images of the same dtype over a 0x5a fill (bevw_remap)."""
    dw, dh = rem.size[2:]
    got = np.full((frames.shape[0], dh, dw), 0x5a5a if frames.dtype == np.uint16 else 0x5a, frames.dtype)
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

    def download(self, shape, dtype):
        raw = self.buf.download((2 * GUARD + self.nbytes + 8,))
        lo, hi = raw[:GUARD + self.shift], raw[GUARD + self.shift + self.nbytes:]
        assert (lo == 0x5a).all() and (hi == 0x5a).all(), "a guard byte was written"
        return raw[GUARD + self.shift:GUARD + self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.download((2 * GUARD + self.nbytes + 8,)) == 0x5a).all())

    def free(self):
        self.buf.free()
