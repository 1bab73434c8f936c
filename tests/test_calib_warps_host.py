"""Host leg of the calibration-side warps (tests/_calib_warps.py has the catalogue, tests/test_calib_warps_gpu.py the GPU leg): nothing here
touches the library under test.

  twins    oracle/bevoracle.c equals oracle/np_twin.py byte for byte over the whole catalogue
  exact    the oracle's Q5 coordinates against exact rational arithmetic (fractions.Fraction) on the doubles of the inverted matrix
  census   every (family, size) reproduces the recorded census, meets its floors and its defining properties"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import np_twin as T
from tests import _calib_warps as CW


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# twins
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CW.FAMILIES)
def test_twin_classic_warp(oracle, name):
    """inverse, coordinates and the warped image, every destination size on SRC and the other sources at (131, 67)"""
    for src, dsize in [(CW.SRC, d) for d in CW.DSIZES] + [(s, (131, 67)) for s in CW.SOURCES]:
        H = CW.homography(name, src, dsize)
        M = oracle.invert3x3(H)
        assert same(M, T.invert3x3(H)), (name, src, dsize)
        xy, a = oracle.perspective_coords(M, dsize)
        txy, ta = T.perspective_coords(M, dsize)
        assert same(xy, txy) and same(a, ta), (name, src, dsize)
        for img in CW.images(src)[:2]:
            assert same(oracle.warp_perspective(img, H, dsize), T.remap_u8(img, xy, a)), (name, src, dsize)


def test_catalogue_tells_block_widths_apart(oracle):
    """The column-block origin enters the fp64 coordinate expression (X0 + M0 x1).  A walk in blocks of 64 columns whatever the height --
    what every destination of 16 rows or more gets -- must differ from the oracle on `tie_tenth` at each of the four sizes whose width is
    not 64, in the coordinates and in image bytes: a kernel that ignored the width would not pass the GPU leg."""
    imgs = CW.images(CW.SRC)
    for dsize in CW.DSIZES:
        H = CW.homography("tie_tenth", CW.SRC, dsize)
        M = oracle.invert3x3(H)
        xy, a = oracle.perspective_coords(M, dsize)
        fxy, fa = T.perspective_coords(M, dsize, block_width=64)
        moved = int(((xy != fxy).any(-1) | (a != fa)).sum())
        changed = sum(int((oracle.remap(img, xy, a) != T.remap_u8(img, fxy, fa)).sum()) for img in imgs)
        if CW.block_width(dsize) in (146, 1024, 257, 68):
            assert moved >= 30 and changed >= 200, (dsize, moved, changed)   # measured: 112 / 66 / 39 / 690 entries, 837 / 497 / 279 / 5411 bytes
        else:
            assert moved == 0 and changed == 0, (dsize, moved, changed)
    assert sum(CW.block_width(d) in (146, 1024, 257, 68) for d in CW.DSIZES) == 4


@pytest.mark.parametrize("name", CW.F32_FAMILIES)
def test_twin_float32_family(oracle, name):
    """the eight members without a fused operation; the twin refuses the others"""
    img = CW.images(CW.SRC)[1]
    try:
        for dsize in CW.EXACT_DSIZES:
            H = CW.homography(name, CW.SRC, dsize)
            M = oracle.invert3x3(H)
            for mode in CW.F32_UNFUSED:
                oracle.set_variant(oracle.VARIANT_WARP, mode)
                assert same(oracle.warp_perspective(img, H, dsize), T.warp_f32(img, M, mode, dsize)), (name, dsize, mode)
    finally:
        oracle.set_variant(oracle.VARIANT_WARP, 0)
    for mode in sorted(set(CW.F32_MODES) - set(CW.F32_UNFUSED)) + [0, 2, 64]:
        with pytest.raises(ValueError):
            T.warp_f32(img, np.eye(3), mode, (8, 8))


def pinhole_maps(oracle, name):
    D, fs, ss, oh, ov = CW.PINHOLE_SETS[name]
    Kd = oracle.camera_mat_dst(CW.PINHOLE_K, CW.FRAME[0], CW.FRAME[1], fs, ss, oh, ov)
    return Kd, oracle.init_undistort_rectify_map(CW.PINHOLE_K, D, Kd, CW.map_size(ss))


@pytest.mark.parametrize("name", list(CW.PINHOLE_SETS))
def test_twin_pinhole_map(oracle, name):
    Kd, (m1, m2) = pinhole_maps(oracle, name)
    D, _, ss = CW.PINHOLE_SETS[name][:3]
    t1, t2 = T.pinhole_map(CW.PINHOLE_K, D, Kd, CW.map_size(ss))
    assert same(m1, t1) and same(m2, t2)
    frame = CW.frames(1)[0]
    assert same(oracle.remap(frame, m1, m2), T.remap_u8(frame, m1, m2))
    sx, sy = m1[..., 0].astype(np.int64), m1[..., 1].astype(np.int64)
    assert ((sx >= 0) & (sx + 1 < CW.FRAME[0]) & (sy >= 0) & (sy + 1 < CW.FRAME[1])).mean() >= 0.25   # the set shows the frame
    if name in CW.PINHOLE_WRAPS:
        # an entry whose integer part does not fit int16 is stored truncated (a wrap), not saturated: rebuild the unwrapped parts in fp64
        # (the lens arithmetic again, without the int32 rounding) and count those beyond the range
        assert wrapped_entries(name, Kd) >= CW.PINHOLE_WRAPS[name]


def wrapped_entries(name, Kd):
    D, _, ss = CW.PINHOLE_SETS[name][:3]
    w, h = CW.map_size(ss)
    d = np.zeros(8)
    d[:len(D)] = D
    K = CW.PINHOLE_K
    x, y = np.meshgrid((np.arange(w) - Kd[0, 2]) / Kd[0, 0], (np.arange(h) - Kd[1, 2]) / Kd[1, 1])
    r2 = x * x + y * y
    with np.errstate(all="ignore"):
        kr = (1 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2) / (1 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2)
        u = K[0, 0] * (x * kr + d[2] * 2 * x * y + d[3] * (r2 + 2 * x * x)) + K[0, 2]
        v = K[1, 1] * (y * kr + d[2] * (r2 + 2 * y * y) + d[3] * 2 * x * y) + K[1, 2]
    return int((~(np.abs(u) < 32767) | ~(np.abs(v) < 32767)).sum())


@pytest.mark.parametrize("name", list(CW.FISHEYE_SETS))
def test_twin_fisheye_map(oracle, name):
    k, fs, ss, oh, ov = CW.FISHEYE_SETS[name]
    K, D = CW.fisheye_calibration(k)
    Kd = oracle.camera_mat_dst(K, CW.FRAME[0], CW.FRAME[1], fs, ss, oh, ov)
    m1, m2 = oracle.fisheye_init_undistort_rectify_map(K, D, Kd, CW.map_size(ss))
    t1, t2 = T.fisheye_map(K, D, Kd, CW.map_size(ss))
    assert same(m1, t1) and same(m2, t2)


def test_twin_resize(oracle):
    cases = CW.resize_cases()
    assert len(cases) >= 40 and any(w * fx > 1024 for w, h, fx, fy in cases)
    for w, h, fx, fy in cases:
        img = np.random.default_rng([w, h]).integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = oracle.resize_linear(img, fx, fy)
        assert (got.shape[1], got.shape[0]) == T.resize_dsize(w, h, fx, fy) == (CW.round_half_even(w * fx), CW.round_half_even(h * fy)), (w, h, fx, fy)
        assert same(got, T.resize_linear(img, fx, fy)), (w, h, fx, fy)
    for (w, h, fx, fy), dsize in CW.RESIZE_TIES.items():
        assert T.resize_dsize(w, h, fx, fy) == dsize == oracle.resize_linear(np.zeros((h, w, 3), np.uint8), fx, fy).shape[1::-1]
    for w, h, fx, fy in CW.RESIZE_EMPTY:
        assert min(T.resize_dsize(w, h, fx, fy)) == 0 and min(oracle.resize_linear(np.zeros((h, w, 3), np.uint8), fx, fy).shape[:2]) == 0


def test_twin_translate(oracle):
    for w, h in CW.TRANSLATE_SIZES:
        img = np.random.default_rng([w, h]).integers(1, 256, (h, w, 3), dtype=np.uint8)
        shifts = CW.translate_shifts(w, h)
        assert len(shifts) >= 20 and max(max(abs(a), abs(b)) for a, b in shifts) == CW.FAR == 2 ** 30
        for sx, sy in shifts:
            got = oracle.translate(img, sx, sy)
            assert same(got, T.translate(img, sx, sy)), (w, h, sx, sy)
            assert bool(got.any()) == (abs(sx) < w and abs(sy) < h), (w, h, sx, sy)


# ---------------------------------------------------------------------------------------------------------------
# the exact leg
# ---------------------------------------------------------------------------------------------------------------
BAR = Fraction(1, 2) + Fraction(1, 10 ** 9)   # half a Q5 unit (the rounding) + 1e-9 for the fp64 evaluation; measured worst excess: see WORST
WORST = 3.5e-13                               # the largest |X - 32 x_exact| - 0.5 over the catalogue, measured 3.42e-13 (horizon_diagonal)


def exact_forms(M, dsize):
    """the three linear forms of the inverse map as Python integers over a common power-of-two denominator: exact"""
    fr = [Fraction(float(v)) for v in np.asarray(M).reshape(9)]
    den = 1
    for f in fr:
        den = max(den, f.denominator)   # denominators of doubles are powers of two: the largest is the common one
    m = [int(f * den) for f in fr]
    assert all(Fraction(a, den) == f for a, f in zip(m, fr))
    x = np.arange(dsize[0], dtype=object)[None, :]
    y = np.arange(dsize[1], dtype=object)[:, None]
    return (m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5], m[6] * x + m[7] * y + m[8])


@pytest.mark.parametrize("name", CW.FAMILIES)
def test_exact_coordinates(oracle, name):
    """|X - 32 x_exact| <= 0.5 + 1e-9 on EVERY entry with W != 0 and |32 x_exact| < 2^20 (X = 32 sx + fx, the oracle's Q5 coordinate);
    (0, 0) with code 0 where W == 0; the saturation carries the sign of x_exact where |x_exact| >= 32769.  x_exact is the quotient of the
    linear forms in exact rational arithmetic on the doubles of the oracle's inverse."""
    worst, held = Fraction(-1), 0
    for dsize in CW.EXACT_DSIZES:
        M = oracle.invert3x3(CW.homography(name, CW.SRC, dsize))
        xy, a = oracle.perspective_coords(M, dsize)
        NX, NY, W = exact_forms(M, dsize)
        zero = (W == 0)
        assert np.array_equal(zero, CW.denominators(M, dsize) == 0), (name, dsize)   # the fp64 denominator vanishes exactly where the exact one does
        assert not xy[zero].any() and not a[zero].any(), (name, dsize)
        code = a.astype(np.int64)
        for N, s, f in ((NX, xy[..., 0].astype(np.int64), code & 31), (NY, xy[..., 1].astype(np.int64), code >> 5)):
            for iy, ix in zip(*np.nonzero(~zero)):
                n, w, X = N[iy, ix], W[iy, ix], 32 * int(s[iy, ix]) + int(f[iy, ix])
                if abs(32 * n) < (2 ** 20) * abs(w):
                    err = Fraction(abs(X * w - 32 * n), abs(w))
                    assert err <= BAR, (name, dsize, ix, iy, float(err))
                    worst, held = max(worst, err), held + 1
                elif abs(n) >= 32769 * abs(w):
                    assert int(s[iy, ix]) == (32767 if (n > 0) == (w > 0) else -32768), (name, dsize, ix, iy)
    print("%s: %d entries held, worst |X - 32 x_exact| - 0.5 = %.3g" % (name, held, float(worst - Fraction(1, 2)) if held else float("nan")))
    assert held > 0 or name in ("far_translate", "singular"), name
    assert worst - Fraction(1, 2) <= Fraction(WORST), (name, float(worst - Fraction(1, 2)))   # the record stays true


# ---------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CW.FAMILIES)
def test_census(oracle, name):
    assert set(CW.CENSUS[name]) == set(CW.DSIZES)
    for dsize in CW.DSIZES:
        got, rec, floor = CW.census(name, dsize), CW.CENSUS[name][dsize], CW.floor(name, dsize)
        assert abs(got["inside"] - rec["inside"]) < 5e-5 and all(got[k] == rec[k] for k in ("border", "saturated", "w_zero", "w_sign")), (name, dsize, got)
        assert got["inside"] >= floor["inside"] and floor["inside"] == CW.round_down(rec["inside"]), (name, dsize)
        for k, v in CW.conditions(name, dsize).items():
            assert (got[k] >= v[1]) if isinstance(v, tuple) else (got[k] == v), (name, dsize, k, v, got[k])
    # the block widths no test ran before are in the catalogue
    assert {CW.block_width(d) for d in CW.DSIZES} >= {146, 1024, 257, 68, 64}


def test_census_controls():
    """the conditions are not vacuous: every horizon and far family has them at the sizes its geometry reaches"""
    assert sum(bool(CW.conditions("horizon_column", d)) for d in CW.DSIZES) == 6      # all but (1, 40)
    assert sum(bool(CW.conditions("horizon_diagonal", d)) for d in CW.DSIZES) == 5    # all but (64, 16) and (1, 40)
    for name in ("far_translate", "far_tiny", "far_huge", "singular") + CW.SHOW:
        assert all(CW.conditions(name, d) for d in CW.DSIZES)
