"""A catalogue of four-camera rigs other than the sample rig, shared by tests/test_rigs_host.py and tests/test_rigs_gpu.py.

Every rig the other tests stitch is workloads.repo_rig() cropped, scaled or shifted: the cameras look the same way, are mounted the same
way up and have the same weak barrel distortion.  `family(name) -> (rig, cfg)` derives rigs from _harness.small_rig() at SMALL_CFG
(320 x 256 frames, 248 x 250 BEV) whose calibration differs in kind: the BEV turned or mirrored, cameras rolled about their axis, strong
minification and magnification, no distortion, strong barrel and pincushion distortion, principal points far off the centre, unequal focal
lengths, a steep perspective, four identical cameras, and other SIZE_SCALE / FOCAL_SCALE values (an undistort grid of another size).

H is a camera's homography from the undistorted image to the BEV, C = (BEV_WIDTH / 2, BEV_HEIGHT / 2) the BEV centre.

`census(name)` measures, from the ORACLE's tables alone, what keeps a family from passing emptily; CENSUS holds the values measured on
the oracle and FLOOR the thresholds the host leg asserts (each the measured value rounded down to the next 0.05).  UNIT_SHARE holds the
share of the BEV the host emulator's units take (tests/native/unit_emulate.cpp on the oracle's tables), UNIT_FLOOR its floors; the GPU leg
holds plan_info()["tiles_staged"] to the same floors.  None of these values comes from the library under test."""
import copy
import math

import numpy as np

from tests._harness import SMALL_CFG, small_rig

CAMS = ("front", "back", "left", "right")
MAGNIFY = 4.0   # the largest whole factor at which every camera keeps a non-fill share of 0.10 (at 5 `right` keeps 0.06, at 8 `left` nothing)

FAMILIES = ("sideways", "reversed", "mirrored", "roll30", "roll90", "minify2", "minify4", "magnify", "pinhole", "barrel_strong", "pincushion",
            "offcentre", "anisotropic", "steep", "same4", "ss13", "fs04")
METHODS = ("sideways", "mirrored", "pincushion", "steep")     # Camera methods and pixel formats run on these
ANALYTIC = ("mirrored", "roll30", "pinhole", "roll90")        # the analytic projection runs on these
ANALYTIC_DROPPED = ("sideways",)   # its specification alone misses the bar against the table path (tests/test_rigs_host.py)
BORDER = ("pincushion", "offcentre", "anisotropic")           # LUT entries outside the frame: the per-tap kernel serves border tiles


def _centre(cfg):
    return cfg["BEV_WIDTH"] / 2.0, cfg["BEV_HEIGHT"] / 2.0


def turn90(cfg):
    """the BEV turned 90 degrees about C with the axis scaling that maps the BEV rectangle onto itself: what was on the left goes to the top"""
    (cx, cy), bw, bh = _centre(cfg), cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    return np.array([[0.0, -bw / bh, cx + cy * bw / bh], [bh / bw, 0.0, cy - cx * bh / bw], [0.0, 0.0, 1.0]])


def turn180(cfg):
    return np.array([[-1.0, 0.0, cfg["BEV_WIDTH"]], [0.0, -1.0, cfg["BEV_HEIGHT"]], [0.0, 0.0, 1.0]])


def mirror(cfg):
    return np.array([[-1.0, 0.0, cfg["BEV_WIDTH"]], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def zoom(cfg, s):
    """scaling by s about C"""
    cx, cy = _centre(cfg)
    return np.array([[s, 0.0, cx * (1 - s)], [0.0, s, cy * (1 - s)], [0.0, 0.0, 1.0]])


def roll(cfg, deg):
    """rotation by deg about the centre of the undistorted image"""
    ux, uy = int(cfg["FRAME_WIDTH"] * cfg["SIZE_SCALE"]) / 2.0, int(cfg["FRAME_HEIGHT"] * cfg["SIZE_SCALE"]) / 2.0
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, ux - c * ux + s * uy], [s, c, uy - s * ux - c * uy], [0.0, 0.0, 1.0]])


def keep_view(cfg, new):
    """T with H' = H @ T showing through the undistorted grid of `new` (other FOCAL_SCALE / SIZE_SCALE) what H shows through cfg's: T takes
    a position of the new undistorted image to the old one.  (SIZE_SCALE 2 -> 1.3 with FOCAL_SCALE 1 -> 0.65: diag(2 / 1.3, 2 / 1.3, 1).)"""
    r = new["FOCAL_SCALE"] / cfg["FOCAL_SCALE"]
    c0 = (cfg["FRAME_WIDTH"] / 2 * cfg["SIZE_SCALE"], cfg["FRAME_HEIGHT"] / 2 * cfg["SIZE_SCALE"])
    c1 = (new["FRAME_WIDTH"] / 2 * new["SIZE_SCALE"], new["FRAME_HEIGHT"] / 2 * new["SIZE_SCALE"])
    return np.array([[1 / r, 0.0, c0[0] - c1[0] / r], [0.0, 1 / r, c0[1] - c1[1] / r], [0.0, 0.0, 1.0]])


def _each(rig, fn):
    return {n: tuple(np.array(a, np.float64) for a in fn(*rig[n])) for n in CAMS}


def _sideways(base, cfg):
    """the BEV turned 90 degrees, every trapezoid served by the neighbouring camera -- and every camera mounted on its side (rolled 90
    degrees about its optical axis).  The turn alone leaves each camera's image axes where the small rig has them relative to the BEV (a
    step along BEV x moves the source more in y on 0.10 of the entries, 0.17 on the small rig): it is the same car drawn pointing right.
    With the roll the family meets its defining property (0.90)."""
    src = dict(front="left", right="front", back="right", left="back")   # trapezoid <- camera
    R, Q = turn90(cfg), roll(cfg, 90.0)
    return {n: (base[s][0].copy(), base[s][1].copy(), R @ base[s][2] @ Q) for n, s in src.items()}


def family(name, magnify=MAGNIFY):
    """-> (rig {camera: (K, D, H)}, cfg); deterministic.  ("small": the small rig itself, the census compares against it.)"""
    base, cfg = small_rig(), dict(SMALL_CFG)
    if name == "small":
        return base, cfg
    if name == "sideways":
        return _sideways(base, cfg), cfg
    if name == "reversed":
        src = dict(front="back", back="front", left="right", right="left")
        return {n: (base[s][0].copy(), base[s][1].copy(), turn180(cfg) @ base[s][2]) for n, s in src.items()}, cfg
    if name == "mirrored":
        src = dict(front="front", back="back", left="right", right="left")
        return {n: (base[s][0].copy(), base[s][1].copy(), mirror(cfg) @ base[s][2]) for n, s in src.items()}, cfg
    if name in ("roll30", "roll90"):
        return _each(base, lambda K, D, H: (K, D, H @ roll(cfg, float(name[4:])))), cfg
    if name in ("minify2", "minify4", "magnify"):
        s = dict(minify2=0.5, minify4=0.25, magnify=magnify)[name]
        return _each(base, lambda K, D, H: (K, D, zoom(cfg, s) @ H)), cfg
    if name == "pinhole":
        return _each(base, lambda K, D, H: (K, np.zeros((4, 1)), H)), cfg
    if name == "barrel_strong":
        return _each(base, lambda K, D, H: (K, D * np.array([[8.0], [20.0], [20.0], [20.0]]), H)), cfg
    if name == "pincushion":
        return _each(base, lambda K, D, H: (K, np.array([[0.3], [0.1], [0.05], [0.02]]), H)), cfg
    if name == "offcentre":
        return _each(base, lambda K, D, H: (K + np.array([[0, 0, 150.0], [0, 0, -120.0], [0, 0, 0]]), D, H)), cfg
    if name == "anisotropic":
        return _each(base, lambda K, D, H: (np.diag([2.0, 0.6, 1.0]) @ K, D, H)), cfg
    if name == "steep":
        return _each(base, lambda K, D, H: (K, D, H * np.array([[1, 1, 1], [1, 1, 1], [1.5, 1.5, 1]]))), cfg
    if name == "same4":
        return {n: tuple(a.copy() for a in base["front"]) for n in CAMS}, cfg
    if name in ("ss13", "fs04"):
        new = dict(cfg, SIZE_SCALE=1.3, FOCAL_SCALE=0.65) if name == "ss13" else dict(cfg, FOCAL_SCALE=0.4)
        rig = _sideways(base, cfg) if name == "ss13" else base
        T = keep_view(cfg, new)
        return _each(rig, lambda K, D, H: (K, D, H @ T)), new
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# the census: from the oracle's tables and masks alone
# ---------------------------------------------------------------------------------------------------------------
_refs = {}


def ref(name, blend=False, balance=False):
    """oracle.RefBevGenerator of a family, built once per (family, blend); the tables do not depend on blend / balance"""
    from oracle import oracle as O

    O.build()
    key = (name, bool(blend))
    if key not in _refs:
        rig, cfg = family(name)
        _refs[key] = O.RefBevGenerator(rig, cfg, blend=blend, balance=False)
    g = _refs[key]
    if bool(balance) != g.balance:
        g = copy.copy(g)
        g.balance = bool(balance)
    return g


def positions(m1, m2):
    """(px, py, fill) of a LUT: sx + fx / 32, sy + fy / 32; fill: the (0, 0), code 0 entries warpPerspective leaves outside the undistort map"""
    code = m2.astype(np.int64) & 1023
    px = m1[..., 0].astype(np.float64) + (code & 31) / 32.0
    py = m1[..., 1].astype(np.float64) + (code >> 5) / 32.0
    return px, py, (m1[..., 0] == 0) & (m1[..., 1] == 0) & (m2 == 0)


STEP = 8   # baseline of the differences: a LUT is a bilinear warp of the undistort map AS AN IMAGE, so the interpolated fraction codes are
           # noise of up to a pixel on a rig that moves the source by half a pixel per BEV pixel; over 8 pixels the small rig's
           # determinant is positive on 0.997 of the entries (0.63 over 1)


def nonfill_shares(gen):
    """per camera: the share of its masked LUT entries that are not fill"""
    out = []
    for cam, mask in zip(gen.cameras, gen.masks):
        m = np.asarray(mask) != 0
        out.append(float((m & ~positions(*cam.bev_maps)[2]).sum()) / max(1, int(m.sum())))
    return out


def jacobian(px, py, ok, k=STEP):
    """differences of the positions over k pixels along BEV x and y where the entry and both far neighbours are `ok` -> (a, b, c, d, sel):
    a = dpx/dx, b = dpx/dy, c = dpy/dx, d = dpy/dy on the [BH - k, BW - k] grid"""
    sel = ok[:-k, :-k] & ok[:-k, k:] & ok[k:, :-k]
    a, c = (px[:-k, k:] - px[:-k, :-k]) / k, (py[:-k, k:] - py[:-k, :-k]) / k
    b, d = (px[k:, :-k] - px[:-k, :-k]) / k, (py[k:, :-k] - py[:-k, :-k]) / k
    return a, b, c, d, sel


def census(name):
    """per family, over the cameras (blend masks: they contain the direct ones):
      nonfill      smallest non-fill share of a camera's masked entries, direct or blend mask
      outside      share of the masked, non-fill entries whose 2 x 2 footprint leaves the frame (all cameras together)
      sideways     share of the masked entries with both neighbours where a step along BEV x moves the source more in y than in x
      det_negative share of those entries whose Jacobian determinant is not positive
      scale        median of sqrt(|det|): source pixels per BEV pixel
      extreme      masked entries that hold +-32767 / -32768 (the int16 saturation of perspective_coords) in the raw perspective
                   coordinates, and whether W changes sign inside a camera's mask"""
    from oracle import oracle as O

    gen = ref(name, blend=True)
    rig, cfg = family(name)
    nonfill = min(nonfill_shares(gen) + nonfill_shares(ref(name, blend=False)))
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    out_n, all_n, side_n, pos_n, jac_n, scales, extreme, wsign = 0, 0, 0, 0, 0, [], 0, False
    for n, cam, mask in zip(CAMS, gen.cameras, gen.masks):
        m = np.asarray(mask) != 0
        px, py, fill = positions(*cam.bev_maps)
        sx, sy = cam.bev_maps[0][..., 0].astype(np.int64), cam.bev_maps[0][..., 1].astype(np.int64)
        outside = (sx < 0) | (sx + 1 > fw - 1) | (sy < 0) | (sy + 1 > fh - 1)
        out_n += int((m & ~fill & outside).sum())
        all_n += int((m & ~fill).sum())
        a, b, c, d, sel = jacobian(px, py, m & ~fill)
        det = (a * d - b * c)[sel]
        side_n += int((np.abs(c) > np.abs(a))[sel].sum())
        pos_n += int((det > 0).sum())
        jac_n += int(sel.sum())
        scales.append(np.sqrt(np.abs(det)))
        xy, _ = O.perspective_coords(O.invert3x3(rig[n][2]), (cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]))
        extreme += int((m & ((np.abs(xy.astype(np.int32)) >= 32767).any(-1))).sum())
        M = O.invert3x3(rig[n][2])
        yy, xx = np.mgrid[0:cfg["BEV_HEIGHT"], 0:cfg["BEV_WIDTH"]].astype(np.float64)
        W = (M[2, 0] * xx + M[2, 1] * yy + M[2, 2])[m]
        wsign = wsign or bool((W > 0).any() and (W < 0).any())
    return dict(nonfill=nonfill, outside=out_n / max(1, all_n), sideways=side_n / max(1, jac_n), det_negative=1.0 - pos_n / max(1, jac_n),
                scale=float(np.median(np.concatenate(scales))) if jac_n else 0.0, extreme=extreme, w_sign_changes=wsign)


def round_down(v, step=0.05):
    """the next multiple of `step` at or below v"""
    return round(math.floor(v / step + 1e-9) * step, 2)


def frames(cfg, n, seed=13):
    """random frames, camera 1 at half brightness: the balance has non-trivial deltas"""
    fr = np.random.default_rng(seed).integers(0, 256, (n, 4, cfg["FRAME_HEIGHT"], cfg["FRAME_WIDTH"], 3), dtype=np.uint8)
    fr[:, 1] //= 2
    return fr


def car(cfg, seed=3):
    """a random sprite on the car rectangle, padded to the BEV"""
    bw, bh, cw, ch = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], cfg["CAR_WIDTH"], cfg["CAR_HEIGHT"]
    out = np.zeros((bh, bw, 3), np.uint8)
    t, l = (bh - ch) // 2, (bw - cw) // 2
    out[t:t + ch, l:l + cw] = np.random.default_rng(seed).integers(0, 256, (ch, cw, 3), dtype=np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------
# recorded values (tests/test_rigs_host.py asserts that a run reproduces them) and the thresholds taken from them
# ---------------------------------------------------------------------------------------------------------------
# census(name) on the oracle's tables (blend masks, differences over STEP pixels)
SMALL_CENSUS = dict(nonfill=0.9942, outside=0.0000, sideways=0.1704, det_negative=0.0026, scale=0.5015, extreme=0, w_sign_changes=False)
CENSUS = {
    "sideways": dict(nonfill=0.7864, outside=0.0000, sideways=0.8998, det_negative=0.0194, scale=0.4852, extreme=36, w_sign_changes=True),
    "reversed": dict(nonfill=0.9947, outside=0.0000, sideways=0.1704, det_negative=0.0028, scale=0.5015, extreme=0, w_sign_changes=False),
    "mirrored": dict(nonfill=0.9947, outside=0.0000, sideways=0.1709, det_negative=0.9969, scale=0.4996, extreme=0, w_sign_changes=False),
    "roll30": dict(nonfill=0.9918, outside=0.0000, sideways=0.3179, det_negative=0.0063, scale=0.5043, extreme=0, w_sign_changes=False),
    "roll90": dict(nonfill=0.9552, outside=0.0000, sideways=0.8233, det_negative=0.0170, scale=0.5074, extreme=0, w_sign_changes=False),
    "minify2": dict(nonfill=1.0000, outside=0.0000, sideways=0.0750, det_negative=0.0657, scale=0.3100, extreme=0, w_sign_changes=False),
    "minify4": dict(nonfill=1.0000, outside=0.0000, sideways=0.0384, det_negative=0.2466, scale=0.2126, extreme=0, w_sign_changes=False),
    "magnify": dict(nonfill=0.2717, outside=0.0000, sideways=0.3115, det_negative=0.6932, scale=0.5206, extreme=218, w_sign_changes=True),
    "pinhole": dict(nonfill=0.9942, outside=0.0000, sideways=0.1662, det_negative=0.0019, scale=0.5174, extreme=0, w_sign_changes=False),
    "barrel_strong": dict(nonfill=0.9942, outside=0.0000, sideways=0.3816, det_negative=0.2184, scale=0.3598, extreme=0, w_sign_changes=False),
    "pincushion": dict(nonfill=0.9942, outside=0.1229, sideways=0.1420, det_negative=0.0002, scale=0.7816, extreme=0, w_sign_changes=False),
    "offcentre": dict(nonfill=0.9942, outside=0.5404, sideways=0.1704, det_negative=0.0026, scale=0.5015, extreme=0, w_sign_changes=False),
    "anisotropic": dict(nonfill=0.9942, outside=0.4923, sideways=0.1650, det_negative=0.0006, scale=0.6654, extreme=0, w_sign_changes=False),
    "steep": dict(nonfill=0.1120, outside=0.0000, sideways=0.1983, det_negative=0.0650, scale=0.6775, extreme=579, w_sign_changes=True),
    "same4": dict(nonfill=0.7425, outside=0.0000, sideways=0.0076, det_negative=0.5553, scale=0.2711, extreme=72, w_sign_changes=True),
    "ss13": dict(nonfill=0.7861, outside=0.0000, sideways=0.8994, det_negative=0.0204, scale=0.4855, extreme=21, w_sign_changes=True),
    "fs04": dict(nonfill=1.0000, outside=0.0000, sideways=0.1730, det_negative=0.0053, scale=0.5048, extreme=0, w_sign_changes=False),
}
# the thresholds: the recorded value rounded down to the next 0.05 -- nonfill for every family, and the value of the property a family is
# named after (minify* / magnify compare `scale` with the small rig's, steep asserts `extreme` / `w_sign_changes`)
FLOOR = {
    "sideways": dict(nonfill=0.75, sideways=0.85),
    "reversed": dict(nonfill=0.95),
    "mirrored": dict(nonfill=0.95, det_negative=0.95),
    "roll30": dict(nonfill=0.95),
    "roll90": dict(nonfill=0.95, sideways=0.80),
    "minify2": dict(nonfill=1.00),
    "minify4": dict(nonfill=1.00),
    "magnify": dict(nonfill=0.25),
    "pinhole": dict(nonfill=0.95),
    "barrel_strong": dict(nonfill=0.95),
    "pincushion": dict(nonfill=0.95, outside=0.10),
    "offcentre": dict(nonfill=0.95, outside=0.50),
    "anisotropic": dict(nonfill=0.95, outside=0.45),
    "steep": dict(nonfill=0.10),
    "same4": dict(nonfill=0.70),
    "ss13": dict(nonfill=0.75, sideways=0.85),
    "fs04": dict(nonfill=1.00),
}
# share of the BEV the host emulator's units take on the oracle's tables, {blend: share} (tests/test_rigs_host.py::test_emulator), and its floors
UNIT_SHARE = {
    "sideways": {False: 1.0000, True: 1.0000},
    "reversed": {False: 1.0000, True: 1.0000},
    "mirrored": {False: 1.0000, True: 1.0000},
    "roll30": {False: 1.0000, True: 1.0000},
    "roll90": {False: 1.0000, True: 1.0000},
    "minify2": {False: 1.0000, True: 1.0000},
    "minify4": {False: 1.0000, True: 1.0000},
    "magnify": {False: 1.0000, True: 1.0000},
    "pinhole": {False: 1.0000, True: 1.0000},
    "barrel_strong": {False: 1.0000, True: 1.0000},
    "pincushion": {False: 0.9009, True: 0.7719},
    "offcentre": {False: 0.8526, True: 0.8526},
    "anisotropic": {False: 0.9009, True: 0.9009},
    "steep": {False: 1.0000, True: 1.0000},
    "same4": {False: 1.0000, True: 1.0000},
    "ss13": {False: 1.0000, True: 1.0000},
    "fs04": {False: 1.0000, True: 1.0000},
}
UNIT_FLOOR = {
    "sideways": {False: 1.00, True: 1.00},
    "reversed": {False: 1.00, True: 1.00},
    "mirrored": {False: 1.00, True: 1.00},
    "roll30": {False: 1.00, True: 1.00},
    "roll90": {False: 1.00, True: 1.00},
    "minify2": {False: 1.00, True: 1.00},
    "minify4": {False: 1.00, True: 1.00},
    "magnify": {False: 1.00, True: 1.00},
    "pinhole": {False: 1.00, True: 1.00},
    "barrel_strong": {False: 1.00, True: 1.00},
    "pincushion": {False: 0.90, True: 0.75},
    "offcentre": {False: 0.85, True: 0.85},
    "anisotropic": {False: 0.90, True: 0.90},
    "steep": {False: 1.00, True: 1.00},
    "same4": {False: 1.00, True: 1.00},
    "ss13": {False: 1.00, True: 1.00},
    "fs04": {False: 1.00, True: 1.00},
}
