"""A catalogue of caller-made remap tables for bevw_remapper_from_maps: maps that fold, mirror, transpose, jump, scatter, collapse to a point,
sit on the frame edge or at the int16 limits.  Shared by the host leg (tests/test_caller_maps_host.py: which path of the plan a map takes)
and the GPU leg (tests/test_caller_maps_gpu.py: what the kernels make of it), so that both speak about the same bytes.

family(name, sw, sh, dw, dh, seed) -> (map1 int16 [dh, dw, 2], map2 uint16 [dh, dw]) is deterministic in its arguments.  map1 holds the
integer source position (sx, sy) of every destination pixel (x, y), map2 the interpolation code.  Unless a family says otherwise map2 is
uniform over all 65,536 values: cv2.remap and the kernels read the low 10 bits only (fx = bits 0..4, fy = bits 5..9).  Every family is a
valid input under the contract of include/bevwarp.h (INTER_LINEAR, BORDER_CONSTANT 0: a tap outside the frame counts 0); none asks a kernel
to read outside a frame.

  scatter      sx uniform in [-3, sw + 3), sy uniform in [-3, sh + 3), independent per pixel
  transpose    (y, x)
  mirror       (sw - 2 - x, y)
  rot180       (sw - 2 - x, sh - 2 - y)
  quadswap     ((x + dw // 2) % dw, (y + dh // 2) % dh): the four quadrants exchanged, discontinuous at the cuts
  constant     (17, 33) everywhere
  stripes      odd rows (sw - 2 - x, y), even rows (x, y)
  rowshuffle   (x, P[y]) with P a random permutation of 0 .. dh - 1
  colshuffle   (P[x], y) with P a random permutation of 0 .. dw - 1
  minify8      (8 x, 8 y): leaves the frame after sw / 8 columns and sh / 8 rows
  magnify16    (x0 + x // 16, y0 + y // 16) with map2 = (x % 16) * 2 + (y % 16) * 2 * 32 (x0, y0 drawn so that the patch lies inside)
  rot45        a rotation by 45 degrees about the frame centre at scale 1: with u = x - dw / 2, v = y - dh / 2 and c = sqrt(1 / 2),
               (floor(sw / 2 + c (u - v)), floor(sh / 2 + c (u + v))); its corners leave the frame when sh < c (dw + dh)
  swirl        a rotation whose angle falls with the distance from the centre: with r = hypot(u, v), R = hypot(dw, dh) / 2,
               t = 3.5 (1 - r / R)^2 and the scales ax = 0.97 sw / dw, ay = 0.97 sh / dh,
               (floor(sw / 2 + ax (u cos t - v sin t)), floor(sh / 2 + ay (u sin t + v cos t)))
  jitter40     the frame less a margin of 8 texels scaled onto the destination, (8 + floor(x (sw - 16) / dw), 8 + floor(y (sh - 16) / dh)),
               with 40 % of the entries (drawn per pixel) displaced by an independent uniform draw from [-12, 12] on each axis.  The units
               take any jitter whose footprints stay inside the frame (their group lists are per texel group, not per row run); what
               sends a base tile to the per-tap kernel is a footprint on the frame border, so the displacement exceeds the margin and the
               tiles along the rim fall to the per-tap kernel while the scattered interior stays with the units
  corner       every entry within 3 rows / 6 columns of a frame edge, on either side of it: sx = sw - 1 - (x // 2) % 6 for odd x,
               (x // 2) % 5 - 1 for even x (every value of -1 .. 3 and sw - 6 .. sw - 1); sy = sh - 1 - (y // 2) % 3 for odd y,
               (y // 2) % 4 - 1 for even y (every value of -1 .. 2 and sh - 3 .. sh - 1)
  extremes     the identity (x, y) with 400 entries (drawn with replacement) replaced, both coordinates, by draws from
               {-32768, 32767, -1, -2, sw - 1, sw, sh - 1, sh}
  strip_w, strip_h, strip_w4   strip-shaped sources at the int16 limit (STRIPS has their sizes).  Per axis of size s, half of the
               entries (drawn per pixel) come from {-2, -1, 0, 1, s - 2, s - 1, s, 32767, -32768}, the rest are uniform in [0, s); s = 32768 wraps to -32768.

One more family stands outside FAMILIES (BATCH_LOOP_FAMILIES: the catalogue's per-family cases do not run it), for the batch-loop tests
(tests/_batch_loops.py), which need whole units without any contributor AND base tiles on the frame border under one map:
  swirl_wide   swirl at the scales ax = 1.6 sw / dw, ay = 1.6 sh / dh: the outer ring of the destination leaves the frame as a whole"""
import numpy as np

SMALL = (256, 192, 160, 120)          # sw, sh, dw, dh
LARGE = (1280, 960, 640, 480)
STRIPS = {"strip_w": (32768, 4, 64, 32), "strip_h": (4, 32768, 64, 32), "strip_w4": (32764, 6, 64, 32)}
LARGE_FAMILIES = ("rot45", "swirl", "jitter40", "minify8")
FAMILIES = ("scatter", "transpose", "mirror", "rot180", "quadswap", "constant", "stripes", "rowshuffle", "colshuffle", "minify8", "magnify16",
            "rot45", "swirl", "jitter40", "corner", "extremes", "strip_w", "strip_h", "strip_w4")
GENERAL = tuple(n for n in FAMILIES if n not in STRIPS)   # the families that take any size
BATCH_LOOP_FAMILIES = ("swirl_wide",)                     # seeded behind FAMILIES; no case list above enumerates them
SEED = 20


def sizes(name):
    """The sizes (sw, sh, dw, dh) at which a family is run: the strips at their own, every other one at SMALL, four of them at LARGE too."""
    if name in STRIPS:
        return [STRIPS[name]]
    return [SMALL] + ([LARGE] if name in LARGE_FAMILIES else [])


def family(name, sw, sh, dw, dh, seed=SEED):
    rng = np.random.default_rng([int(seed), (FAMILIES + BATCH_LOOP_FAMILIES).index(name)])
    map2 = rng.integers(0, 65536, (dh, dw)).astype(np.uint16)
    y, x = np.mgrid[0:dh, 0:dw]
    if name == "scatter":
        sx, sy = rng.integers(-3, sw + 3, (dh, dw)), rng.integers(-3, sh + 3, (dh, dw))
    elif name == "transpose":
        sx, sy = y, x
    elif name == "mirror":
        sx, sy = sw - 2 - x, y
    elif name == "rot180":
        sx, sy = sw - 2 - x, sh - 2 - y
    elif name == "quadswap":
        sx, sy = (x + dw // 2) % dw, (y + dh // 2) % dh
    elif name == "constant":
        sx, sy = np.full((dh, dw), 17), np.full((dh, dw), 33)
    elif name == "stripes":
        sx, sy = np.where(y % 2 == 1, sw - 2 - x, x), y
    elif name == "rowshuffle":
        sx, sy = x, rng.permutation(dh)[y]
    elif name == "colshuffle":
        sx, sy = rng.permutation(dw)[x], y
    elif name == "minify8":
        sx, sy = 8 * x, 8 * y
    elif name == "magnify16":
        x0, y0 = int(rng.integers(0, sw - dw // 16 - 1)), int(rng.integers(0, sh - dh // 16 - 1))
        sx, sy = x0 + x // 16, y0 + y // 16
        map2 = ((x % 16) * 2 + (y % 16) * 2 * 32).astype(np.uint16)
    elif name == "rot45":
        u, v, c = x - dw / 2, y - dh / 2, np.sqrt(0.5)
        sx, sy = np.floor(sw / 2 + c * (u - v)), np.floor(sh / 2 + c * (u + v))
    elif name in ("swirl", "swirl_wide"):
        u, v = x - dw / 2, y - dh / 2
        t = 3.5 * (1 - np.hypot(u, v) / (np.hypot(dw, dh) / 2)) ** 2
        scale = 0.97 if name == "swirl" else 1.6
        ax, ay = scale * sw / dw, scale * sh / dh
        sx, sy = np.floor(sw / 2 + ax * (u * np.cos(t) - v * np.sin(t))), np.floor(sh / 2 + ay * (u * np.sin(t) + v * np.cos(t)))
    elif name == "jitter40":
        hit = rng.random((dh, dw)) < 0.4
        sx = 8 + x * (sw - 16) // dw + np.where(hit, rng.integers(-12, 13, (dh, dw)), 0)
        sy = 8 + y * (sh - 16) // dh + np.where(hit, rng.integers(-12, 13, (dh, dw)), 0)
    elif name == "corner":
        sx = np.where(x % 2 == 1, sw - 1 - (x // 2) % 6, (x // 2) % 5 - 1)
        sy = np.where(y % 2 == 1, sh - 1 - (y // 2) % 3, (y // 2) % 4 - 1)
    elif name == "extremes":
        m = np.stack([x, y], -1).reshape(-1, 2)
        m[rng.integers(0, dh * dw, 400)] = rng.choice([-32768, 32767, -1, -2, sw - 1, sw, sh - 1, sh], (400, 2))
        sx, sy = m[:, 0].reshape(dh, dw), m[:, 1].reshape(dh, dw)
    elif name in STRIPS:
        def pick(s):
            edge = rng.choice([-2, -1, 0, 1, s - 2, s - 1, s, 32767, -32768], (dh, dw))
            return np.where(rng.random((dh, dw)) < 0.5, edge, rng.integers(0, s, (dh, dw)))
        sx, sy = pick(sw), pick(sh)
    else:
        raise ValueError(name)
    m1 = np.stack([sx, sy], -1)
    if name in STRIPS:
        m1 = (m1 + 32768) % 65536 - 32768   # s = 32768 itself is no int16 value: it wraps to -32768, as a caller's cast would make it
    assert m1.min() >= -32768 and m1.max() <= 32767, name
    return np.ascontiguousarray(m1.astype(np.int16)), np.ascontiguousarray(map2)


def numpy_remap(img, map1, map2):
    """The fixed-point formula of cv2.remap (INTER_LINEAR, BORDER_CONSTANT 0) in plain NumPy, int64: (sum p wx wy + 512) >> 10 with 5-bit
    weights from the low 10 bits of map2 and a tap outside the frame counted as 0.  img uint8 [sh, sw, 3] -> uint8 [dh, dw, 3]."""
    sh, sw = img.shape[:2]
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    fx, fy = (map2 & 31).astype(np.int64), ((map2 >> 5) & 31).astype(np.int64)
    acc = np.zeros(map2.shape + (3,), np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            tx, ty = sx + dx, sy + dy
            inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
            p = img[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int64)
            acc += p * (wx * wy * inside)[..., None]
    return ((acc + 512) >> 10).astype(np.uint8)


def child_cases():
    """(family, size, input format) of the plan-off child of tests/test_caller_maps_gpu.py: every family at its first size."""
    return [(name, sizes(name)[0], inp) for name in FAMILIES for inp in ("bgr", "nv12", "yuyv")]
