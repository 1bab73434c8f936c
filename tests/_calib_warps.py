"""A catalogue of inputs for the calibration-side warps, shared by tests/test_calib_warps_host.py and tests/test_calib_warps_gpu.py:
homographies for cv2.warpPerspective (k_warp_perspective, classic and the float32 family), lens sets for the pinhole and fisheye map
builders (k_pinhole_map, k_fisheye_map), resize cases (k_resize_linear) and translate cases (k_translate).  Everything is deterministic.

homography(name, src, dsize) -> H, the FORWARD 3 x 3 matrix cv2.warpPerspective takes (the kernels invert it).  src = (sw, sh) and
dsize = (dw, dh) in pixels.  The families of SHOW are meant to show the image: they are A in normalised coordinates, H = D A N with N
taking the source rectangle onto [-1, 1]^2 and D taking [-1, 1]^2 onto the destination rectangle (pixel centres at half-integers: the one
column of a 1 x 40 destination is u = 0), so a wide, flat destination is not mostly empty.  The others are the matrix as written, whatever the sizes:

  identity, shift_int (-5, -3), shift_half (0.5, -0.5), shift_64th (1/64, -3/64: 32 x - 0.5 and 32 y + 1.5, exact Q5 ties)
  tie_tenth         [[10, 0, -10/64], [0, 10, -10/64], [0, 0, 1]]: the source position is 0.1 x + 1/64, so 32 times it is a Q5 tie in exact
                    arithmetic at every fifth column and row, and in fp64 it lands a rounding error above or below the tie: which side depends
                    on where the column block starts (X0 + M0 x1), so this family tells one block width from another
  fit, rot30, rot90, rot180, mirror (negative determinant), minify8, magnify8, steep (W = 1 - 0.6 u - 0.3 v in [0.1, 1.9] over the
      destination: sign-stable), mild (the third matrix of test_excalibrator_warp, then the fit)                              -- SHOW
  horizon_column    [[1, 0, 0], [0, 1, 0], [1/32, 0, 1/32]]: the cofactor inverse is exactly [[1, 0, 0], [0, 1, 0], [-1, 0, 32]], W = 32 - x
                    is exactly 0 on the column x = 32 and changes sign there
  horizon_diagonal  the cofactor inverse of [[1, .1, 0], [.05, 1, 0], [-.01, -.02, 1]]: W = 1 - 0.01 x - 0.02 y up to rounding, a
                    diagonal horizon along x + 2 y = 100
  far_translate     a translation by (1e7, -1e7): every coordinate beyond the int16 range, inside the int32 one
  far_tiny          diag(1e-12, 1e-12, 1): every coordinate but those of x = 0 / y = 0 at the int32 clamp
  far_huge          diag(1e300, 1e-300, 1): x collapses to 0, y is at the clamp from the second row on
  singular          [[1, 2, 3], [2, 4, 6], [1, 1, 1]]: the inverse is zero-filled, W == 0 everywhere, every pixel is src[0, 0]
  near_singular     the same with 4 + 2^-20 in the middle: determinant -2^-19, inverse entries of about 1e6

census(name, dsize) measures, from the ORACLE's coordinates alone and on the SRC source, what keeps a (family, size) from passing emptily;
CENSUS holds the values measured on the oracle, floor(name, dsize) the thresholds the host leg asserts (a share rounded down to the next
0.05, a count as it is), conditions(name, dsize) the defining properties.  None of these values comes from the library under test."""
import math

import numpy as np

SRC = (96, 64)                                                   # (sw, sh): every family runs on it
SOURCES = ((97, 65), (1, 1), (1, 40), (37, 2))                   # rows that are no dword multiples; one texel; one column; two rows
DSIZES = ((300, 7), (1100, 1), (257, 3), (700, 15), (131, 67), (64, 16), (1, 40))   # block widths 146, 1024, 257, 68, 64, 64, 1
EXACT_DSIZES = ((131, 67), (300, 7))
SHOW = ("fit", "rot30", "rot90", "rot180", "mirror", "minify8", "magnify8", "steep", "mild")
FAMILIES = ("identity", "shift_int", "shift_half", "shift_64th", "tie_tenth") + SHOW + (
    "horizon_column", "horizon_diagonal", "far_translate", "far_tiny", "far_huge", "singular", "near_singular")
ON_SOURCES = ("identity", "shift_half", "fit", "rot30", "mirror", "magnify8", "steep")   # run on SOURCES too: they still show the image
F32_FAMILIES = ("mild", "rot30", "horizon_diagonal", "minify8", "far_translate")
F32_MODES = tuple(range(1, 64, 2))                               # all 32 members
F32_UNFUSED = (1, 9, 17, 25, 33, 41, 49, 57)                     # the members np_twin.warp_f32 states
BATCH = 3


def cofactor_inverse(m):
    """the 3 x 3 inverse by cofactors in Python floats (deterministic on every machine, unlike a LAPACK call)"""
    (a, b, c), (d, e, f), (g, h, i) = [[float(v) for v in r] for r in m]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    s = 1.0 / det
    return np.array([[(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s],
                     [(f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s],
                     [(d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s]])


def _shift(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def _rot(deg):
    c, s = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0)}.get(deg, (math.cos(math.radians(deg)), math.sin(math.radians(deg))))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


MILD = np.array([[0.9, 0.2, -3.0], [-0.1, 1.1, 2.0], [1e-3, -2e-3, 1.0]])


def homography(name, src=SRC, dsize=(131, 67)):
    (sw, sh), (dw, dh) = src, dsize
    N = np.array([[2.0 / sw, 0.0, 1.0 / sw - 1.0], [0.0, 2.0 / sh, 1.0 / sh - 1.0], [0.0, 0.0, 1.0]])
    D = np.array([[dw / 2.0, 0.0, dw / 2.0 - 0.5], [0.0, dh / 2.0, dh / 2.0 - 0.5], [0.0, 0.0, 1.0]])
    if name == "identity":
        return np.eye(3)
    if name == "shift_int":
        return _shift(-5.0, -3.0)
    if name == "shift_half":
        return _shift(0.5, -0.5)
    if name == "shift_64th":
        return _shift(1.0 / 64, -3.0 / 64)
    if name == "tie_tenth":
        return np.array([[10.0, 0.0, -10.0 / 64], [0.0, 10.0, -10.0 / 64], [0.0, 0.0, 1.0]])
    if name == "fit":
        return D @ N
    if name in ("rot30", "rot90", "rot180"):
        return D @ _rot(int(name[3:])) @ N
    if name == "mirror":
        return D @ np.diag([-1.0, 1.0, 1.0]) @ N
    if name == "minify8":
        return D @ np.diag([0.125, 0.125, 1.0]) @ N
    if name == "magnify8":
        return D @ np.diag([8.0, 8.0, 1.0]) @ N
    if name == "steep":
        return D @ np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.3, 1.0]]) @ N
    if name == "mild":
        return np.diag([dw / sw, dh / sh, 1.0]) @ MILD
    if name == "horizon_column":
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0 / 32, 0.0, 1.0 / 32]])
    if name == "horizon_diagonal":
        return cofactor_inverse([[1.0, 0.1, 0.0], [0.05, 1.0, 0.0], [-0.01, -0.02, 1.0]])
    if name == "far_translate":
        return _shift(1e7, -1e7)
    if name == "far_tiny":
        return np.diag([1e-12, 1e-12, 1.0])
    if name == "far_huge":
        return np.diag([1e300, 1e-300, 1.0])
    if name == "singular":
        return np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 1.0, 1.0]])
    if name == "near_singular":
        return np.array([[1.0, 2.0, 3.0], [2.0, 4.0 + 2.0 ** -20, 6.0], [1.0, 1.0, 1.0]])
    raise KeyError(name)


def images(src, n=BATCH, seed=5):
    """n distinct random images [n, sh, sw, 3]"""
    return np.random.default_rng([seed, src[0], src[1]]).integers(0, 256, (n, src[1], src[0], 3), dtype=np.uint8)


def block_width(dsize):
    """columns per block of the destination walk (the block origin enters the fp64 expression)"""
    return min(1024 // min(16, dsize[1]), dsize[0])


# ---------------------------------------------------------------------------------------------------------------
# the census: from the oracle's inverse and coordinates alone
# ---------------------------------------------------------------------------------------------------------------
def denominators(M, dsize):
    """W of every destination pixel in the association of the block walk, W0 + M6 x1 (fp64)"""
    dw, dh = dsize
    bw = block_width(dsize)
    xs = np.arange(dw)
    x0, x1 = (xs // bw * bw).astype(np.float64)[None, :], (xs % bw).astype(np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    return (M[2, 0] * x0 + M[2, 1] * y + M[2, 2]) + M[2, 0] * x1


def census(name, dsize, src=SRC):
    """inside     share of the destination pixels with at least one of their four taps inside the source
    border     pixels with a tap inside and a tap outside (border footprints)
    saturated  entries that hold -32768 or 32767 in a coordinate (the int16 saturation of the coordinates)
    w_zero     entries with W == 0
    w_sign     whether W is positive on one entry and negative on another"""
    from oracle import oracle as O

    O.build()
    sw, sh = src
    M = O.invert3x3(homography(name, src, dsize))
    xy, _ = O.perspective_coords(M, dsize)
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    any_in = (sx >= -1) & (sx < sw) & (sy >= -1) & (sy < sh)
    all_in = (sx >= 0) & (sx + 1 < sw) & (sy >= 0) & (sy + 1 < sh)
    W = denominators(M, dsize)
    return dict(inside=float(any_in.mean()), border=int((any_in & ~all_in).sum()), saturated=int(((xy == -32768) | (xy == 32767)).any(-1).sum()),
                w_zero=int((W == 0).sum()), w_sign=bool((W > 0).any() and (W < 0).any()))


def round_down(v, step=0.05):
    """the next multiple of `step` at or below v"""
    return round(math.floor(v / step + 1e-9) * step, 2)


def floor(name, dsize):
    """what the host leg asserts of census(name, dsize): the recorded share rounded down to the next 0.05, the recorded counts"""
    c = CENSUS[name][tuple(dsize)]
    return dict(c, inside=round_down(c["inside"]))


def conditions(name, dsize):
    """the defining properties of a (family, size) as {census key: required value or ('>=', bound)}, from the geometry alone:
    the column horizon needs the column x = 32 and one on either side of it; the diagonal one needs pixels on both sides of
    x + 2 y = 100; far_tiny keeps the pixel (0, 0) alone (row 0 and column 0 keep one coordinate at 0, the other one is saturated);
    far_huge keeps row 0 whole (y = 0 stays 0, and 1e-300 x rounds to 0)"""
    dw, dh = dsize
    n = dw * dh
    if name == "horizon_column" and dw > 33:
        return dict(w_zero=dh, w_sign=True)
    if name == "horizon_diagonal" and (dw - 1) + 2 * (dh - 1) > 100:
        return dict(w_sign=True, saturated=(">=", 1))
    if name == "far_translate":
        return dict(saturated=n, inside=0.0)
    if name == "far_tiny":
        return dict(saturated=n - 1)
    if name == "far_huge":
        return dict(saturated=dw * (dh - 1))
    if name == "singular":
        return dict(w_zero=n, inside=1.0, border=0)
    if name in SHOW or name in ("identity", "shift_int", "shift_half", "shift_64th", "tie_tenth"):
        return dict(inside=(">=", 1.0 / n), w_zero=0, w_sign=False)   # at least one pixel shows the image, no horizon
    return {}


# ---------------------------------------------------------------------------------------------------------------
# lens sets of the map builders: 320 x 256 frames
# ---------------------------------------------------------------------------------------------------------------
FRAME = (320, 256)
PINHOLE_K = np.array([[205.0, 0.0, 163.825], [0.0, 203.875, 125.175], [0.0, 0.0, 1.0]])
# name -> (D, FOCAL_SCALE, SIZE_SCALE, offset_h, offset_v)
PINHOLE_SETS = {
    "d0": ([], 1.0, 1.0, 0.0, 0.0),
    "d4": ([0.05, -0.01, 0.0, 0.0], 1.0, 1.0, 0.0, 0.0),
    "d5": ([-0.31, 0.12, 0.0011, -0.0007, -0.02], 0.5, 1.0, 0.0, 0.0),
    "d8": ([-0.2, 0.05, 0.001, 0.002, 0.01, 0.02, -0.01, 0.003], 0.5, 1.0, 0.0, 0.0),
    "barrel_fold": ([-0.9, 0.0, 0.0, 0.0, 0.0], 0.5, 1.0, 0.0, 0.0),                     # k1 = -0.9: the image folds over inside the grid
    "tangential": ([-0.1, 0.02, 0.2, -0.15, 0.0], 0.6, 1.0, 0.0, 0.0),
    "ss17_offset": ([-0.31, 0.12, 0.0011, -0.0007, -0.02], 0.8, 1.7, -33.5, 21.25),
    "ss05": ([-0.31, 0.12, 0.0011, -0.0007, -0.02], 0.5, 0.5, 0.0, 0.0),
    "rational_pole": ([0.0, 0.0, 0.0, 0.0, 0.0, -2.0, 0.0, 0.0], 0.5, 1.0, 0.0, 0.0),  # 1 - 2 r^2 passes through zero at r^2 = 0.5
    "extreme": ([2.0, 3.0, 0.0, 0.0, 5.0], 0.05, 1.0, 0.0, 0.0),                        # u * 32 beyond int32 on most of the grid
}
PINHOLE_WRAPS = {"rational_pole": 1, "extreme": 50000}   # at least so many entries whose iu >> 5 or iv >> 5 does not fit int16
FISHEYE_SETS = {"x%d_%s_ss%s" % (k, "off" if off[0] else "ctr", str(ss).replace(".", "")): (float(k), 0.5 if ss == 1.0 else 1.0, ss) + off
                for k in (0, 1, 8) for off in ((0.0, 0.0), (-33.5, 21.25)) for ss in (1.0, 1.7, 0.5)}   # name -> (D factor, FOCAL_SCALE, SIZE_SCALE, offsets)


def fisheye_calibration(factor):
    """K and D of the sample rig's front camera at 320 x 256 frames, D times `factor`"""
    from tests._harness import small_rig

    K, D, _ = small_rig()["front"]
    return np.array(K, np.float64), np.array(D, np.float64).reshape(-1) * factor


def map_size(ss):
    return int(FRAME[0] * ss), int(FRAME[1] * ss)


def frames(n=2, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (n, FRAME[1], FRAME[0], 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# resize and translate cases
# ---------------------------------------------------------------------------------------------------------------
RESIZE_FACTORS = (0.1, 0.23, 0.5, 0.77, 1.0, 1.41, 2.0, 3.3, 17.0)
RESIZE_PAIRS = ((0.1, 7.0), (7.0, 0.1))
RESIZE_SOURCES = ((1, 1), (2, 2), (1, 9), (9, 1), (5, 7), (61, 83))                  # (w, h)
RESIZE_WIDE = ((61, 83), 17.0, 0.1)            # 61 * 17 = 1037 columns: five thread blocks in x, the last one partial
# w * fx exactly k + 0.5: cvRound goes to the even neighbour.  (w, h, fx, fy) -> dsize
RESIZE_TIES = {(5, 7, 0.5, 0.5): (2, 4), (7, 5, 0.5, 0.5): (4, 2), (3, 1, 0.5, 1.5): (2, 2), (1, 3, 2.5, 0.5): (2, 2)}
RESIZE_EMPTY = ((2, 2, 0.1, 1.0), (5, 7, 1.0, 0.07), (1, 1, 0.5, 0.5))   # 0.2 -> 0, 0.49 -> 0, 0.5 -> 0 (the tie goes to the even 0): refused


def resize_cases():
    """every (w, h, fx, fy) of the catalogue whose destination is not empty"""
    out = []
    for (w, h) in RESIZE_SOURCES:
        for f in RESIZE_FACTORS:
            out.append((w, h, f, f))
        for fx, fy in RESIZE_PAIRS:
            out.append((w, h, fx, fy))
    out.append((RESIZE_WIDE[0][0], RESIZE_WIDE[0][1], RESIZE_WIDE[1], RESIZE_WIDE[2]))
    out += list(RESIZE_TIES)
    return [c for c in out if min(round_half_even(c[0] * c[2]), round_half_even(c[1] * c[3])) > 0]


def round_half_even(v):
    """half to even in exact arithmetic on the double v (Python's round)"""
    return int(round(v))


TRANSLATE_SIZES = ((1, 1), (257, 3), (300, 7), (97, 65))                             # (w, h)
FAR = 2 ** 30   # the largest power of two at which x - shift overflows an int on neither side


def translate_shifts(w, h):
    """(shift_x, shift_y): every axis through 0, +-1, +-(n - 1), +-n, +-(3 n + 1) and +-2^30, the two axes paired with mixed signs"""
    ax = lambda n: [0, 1, -1, n - 1, -(n - 1), n, -n, 3 * n + 1, -(3 * n + 1), FAR, -FAR]
    xs, ys = ax(w), ax(h)
    out = [(sx, 0) for sx in xs] + [(0, sy) for sy in ys]
    out += [(xs[i], ys[(i * 3 + 2) % len(ys)]) for i in range(len(xs))] + [(xs[i], -ys[i]) for i in range(1, 5)]
    return sorted(set(out))


# ---------------------------------------------------------------------------------------------------------------
# recorded values (tests/test_calib_warps_host.py asserts that a run reproduces them)
# ---------------------------------------------------------------------------------------------------------------
# census(name, dsize) on SRC, per family and destination size
CENSUS = {
    "identity": {
        (300, 7): dict(inside=0.3200, border=7, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0873, border=1, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.3735, border=3, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.1371, border=15, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.7000, border=159, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "shift_int": {
        (300, 7): dict(inside=0.3033, border=7, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0827, border=1, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.3541, border=3, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.1300, border=15, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.6324, border=151, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "shift_half": {
        (300, 7): dict(inside=0.3233, border=14, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0882, border=2, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.3774, border=6, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.1386, border=30, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.7073, border=223, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=16, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=40, saturated=0, w_zero=0, w_sign=False),
    },
    "shift_64th": {
        (300, 7): dict(inside=0.3200, border=7, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0873, border=1, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.3735, border=3, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.1371, border=15, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.7000, border=159, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "tie_tenth": {
        (300, 7): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.8727, border=10, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "fit": {
        (300, 7): dict(inside=1.0000, border=28, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=12, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=6, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=120, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=392, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "rot30": {
        (300, 7): dict(inside=0.8652, border=46, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.8859, border=22, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.8565, border=226, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.8561, border=193, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.8574, border=22, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "rot90": {
        (300, 7): dict(inside=1.0000, border=28, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=17, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=12, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=165, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=134, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=16, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "rot180": {
        (300, 7): dict(inside=1.0000, border=28, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=12, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=6, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=120, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=392, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "mirror": {
        (300, 7): dict(inside=1.0000, border=28, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=12, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=6, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=120, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=392, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "minify8": {
        (300, 7): dict(inside=0.0181, border=0, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.1255, border=2, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.0428, border=2, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.0084, border=2, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.0174, border=0, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.0156, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.1500, border=2, saturated=0, w_zero=0, w_sign=False),
    },
    "magnify8": {
        (300, 7): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "steep": {
        (300, 7): dict(inside=0.7557, border=22, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.8145, border=5, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.7691, border=6, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.7545, border=114, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.7528, border=88, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.7539, border=12, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.9000, border=1, saturated=0, w_zero=0, w_sign=False),
    },
    "mild": {
        (300, 7): dict(inside=0.8848, border=61, saturated=0, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.7673, border=122, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.8612, border=37, saturated=0, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.8927, border=225, saturated=0, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.8989, border=149, saturated=0, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.8945, border=21, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.3750, border=5, saturated=0, w_zero=0, w_sign=False),
    },
    "horizon_column": {
        (300, 7): dict(inside=0.1100, border=0, saturated=0, w_zero=7, w_sign=True),
        (1100, 1): dict(inside=0.0300, border=0, saturated=0, w_zero=1, w_sign=True),
        (257, 3): dict(inside=0.1284, border=0, saturated=0, w_zero=3, w_sign=True),
        (700, 15): dict(inside=0.0471, border=0, saturated=0, w_zero=15, w_sign=True),
        (131, 67): dict(inside=0.2516, border=1, saturated=0, w_zero=67, w_sign=True),
        (64, 16): dict(inside=0.5156, border=0, saturated=0, w_zero=16, w_sign=True),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
    "horizon_diagonal": {
        (300, 7): dict(inside=0.1533, border=0, saturated=7, w_zero=0, w_sign=True),
        (1100, 1): dict(inside=0.0445, border=0, saturated=1, w_zero=0, w_sign=True),
        (257, 3): dict(inside=0.1868, border=0, saturated=3, w_zero=0, w_sign=True),
        (700, 15): dict(inside=0.0600, border=0, saturated=15, w_zero=0, w_sign=True),
        (131, 67): dict(inside=0.1044, border=6, saturated=51, w_zero=0, w_sign=True),
        (64, 16): dict(inside=0.6484, border=0, saturated=0, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.7250, border=1, saturated=0, w_zero=0, w_sign=False),
    },
    "far_translate": {
        (300, 7): dict(inside=0.0000, border=0, saturated=2100, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0000, border=0, saturated=1100, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.0000, border=0, saturated=771, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.0000, border=0, saturated=10500, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.0000, border=0, saturated=8777, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.0000, border=0, saturated=1024, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.0000, border=0, saturated=40, w_zero=0, w_sign=False),
    },
    "far_tiny": {
        (300, 7): dict(inside=0.0005, border=0, saturated=2099, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=0.0009, border=0, saturated=1099, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.0013, border=0, saturated=770, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.0001, border=0, saturated=10499, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.0001, border=0, saturated=8776, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.0010, border=0, saturated=1023, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.0250, border=0, saturated=39, w_zero=0, w_sign=False),
    },
    "far_huge": {
        (300, 7): dict(inside=0.1429, border=0, saturated=1800, w_zero=0, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=0, saturated=0, w_zero=0, w_sign=False),
        (257, 3): dict(inside=0.3333, border=0, saturated=514, w_zero=0, w_sign=False),
        (700, 15): dict(inside=0.0667, border=0, saturated=9800, w_zero=0, w_sign=False),
        (131, 67): dict(inside=0.0149, border=0, saturated=8646, w_zero=0, w_sign=False),
        (64, 16): dict(inside=0.0625, border=0, saturated=960, w_zero=0, w_sign=False),
        (1, 40): dict(inside=0.0250, border=0, saturated=39, w_zero=0, w_sign=False),
    },
    "singular": {
        (300, 7): dict(inside=1.0000, border=0, saturated=0, w_zero=2100, w_sign=False),
        (1100, 1): dict(inside=1.0000, border=0, saturated=0, w_zero=1100, w_sign=False),
        (257, 3): dict(inside=1.0000, border=0, saturated=0, w_zero=771, w_sign=False),
        (700, 15): dict(inside=1.0000, border=0, saturated=0, w_zero=10500, w_sign=False),
        (131, 67): dict(inside=1.0000, border=0, saturated=0, w_zero=8777, w_sign=False),
        (64, 16): dict(inside=1.0000, border=0, saturated=0, w_zero=1024, w_sign=False),
        (1, 40): dict(inside=1.0000, border=0, saturated=0, w_zero=40, w_sign=False),
    },
    "near_singular": {
        (300, 7): dict(inside=0.0014, border=0, saturated=0, w_zero=1, w_sign=True),
        (1100, 1): dict(inside=0.0000, border=0, saturated=0, w_zero=0, w_sign=True),
        (257, 3): dict(inside=0.0013, border=0, saturated=0, w_zero=1, w_sign=True),
        (700, 15): dict(inside=0.0007, border=4, saturated=0, w_zero=1, w_sign=True),
        (131, 67): dict(inside=0.0038, border=30, saturated=0, w_zero=1, w_sign=True),
        (64, 16): dict(inside=0.0068, border=4, saturated=0, w_zero=1, w_sign=True),
        (1, 40): dict(inside=0.0000, border=0, saturated=0, w_zero=0, w_sign=False),
    },
}
