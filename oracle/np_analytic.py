"""TEST INFRASTRUCTURE (never imported by the product): NumPy fp64 statement of the ANALYTIC projection mode
(bevw_set_projection(BEVW_PROJ_ANALYTIC)).

The reference has no such path -- its per-frame work is a table-driven cv2.remap (surroundBEV.py:116-117) -- so this is not
a restatement of reference code but the specification of the mode, written with the reference's own formulas:

    BEV pixel (x, y)  --H^-1-->  undistorted pixel (u, v)            ExCalibrator / warpPerspective geometry, surroundBEV.py:113-114
    (u, v)  --K'^-1, fisheye model (theta_d = theta (1 + k1 theta^2 + ...)), K-->  raw position (px, py)
                                                                     cv2.fisheye.initUndistortRectifyMap, surroundBEV.py:99-102
    bilinear interpolation of the 4 texels in fp64, round half to even, BORDER_CONSTANT 0 per tap
    zero where (u, v) leaves the undistorted image (warp_homography of an image is 0 there)

then the reference's own mask / blend weight / saturating sums / car.  With balance= the chain is the reference's
(RefBevGenerator.__call__): oracle.luminance_balance on the four frames, sample and mask, the three saturating sums,
oracle.color_balance, the car.  (The kernel shifts the luminance of every fetched texel instead of the whole frame first:
the same bytes reach the interpolation.)"""
import copy

import numpy as np

from . import oracle


def positions(K, D, H, cfg, dtype=np.float64):
    """(u, v, px, py, Wd) [BH, BW] of one camera, before any validity test, every operation in `dtype`.  float64 is the
    specification; float32 (parameters rounded once, the inverse homography inverted in fp64 first, as the library does) is
    what the tests measure the fp32 mode's position error with."""
    K, D, H = (np.asarray(a, np.float64) for a in (K, D, H))
    D = D.ravel()
    fw, fh, ss = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["SIZE_SCALE"]
    bw, bh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    Kd = oracle.camera_mat_dst(K, fw, fh, cfg["FOCAL_SCALE"], ss).astype(dtype)
    M = oracle.invert3x3(H).astype(dtype)
    K, D = K.astype(dtype), D.astype(dtype)
    one = dtype(1)
    yy, xx = np.mgrid[0:bh, 0:bw].astype(dtype)
    X = M[0, 0] * xx + M[0, 1] * yy + M[0, 2]
    Y = M[1, 0] * xx + M[1, 1] * yy + M[1, 2]
    Wd = M[2, 0] * xx + M[2, 1] * yy + M[2, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, v = X / Wd, Y / Wd
        xn, yn = (u - Kd[0, 2]) / Kd[0, 0], (v - Kd[1, 2]) / Kd[1, 1]
        r = np.sqrt(xn * xn + yn * yn)
        theta = np.arctan(r)
        t2 = theta * theta
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        theta_d = theta * (one + D[0] * t2 + D[1] * t4 + D[2] * t6 + D[3] * t8)
        scale = np.where(r == 0, one, theta_d / np.where(r == 0, one, r))
        px = K[0, 0] * xn * scale + K[0, 2]
        py = K[1, 1] * yn * scale + K[1, 2]
    return u, v, px, py, Wd


def project(K, D, H, cfg):
    """(px, py, valid) float64 [BH, BW]: raw-frame position sampled by every BEV pixel of one camera."""
    fw, fh, ss = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["SIZE_SCALE"]
    uw, uh = int(fw * ss), int(fh * ss)
    u, v, px, py, Wd = positions(K, D, H, cfg)
    with np.errstate(invalid="ignore"):
        valid = (Wd != 0) & (u >= 0) & (u <= uw - 1) & (v >= 0) & (v <= uh - 1)
        valid &= (px > -1.0) & (px < fw) & (py > -1.0) & (py < fh)
    return np.where(valid, px, 0.0), np.where(valid, py, 0.0), valid


def edge_band(K, D, H, cfg, eps):
    """bool [BH, BW]: pixels whose fp64 u, v, px or py lies within `eps` of one of project()'s validity comparisons -- where an
    arithmetic with position errors below eps may decide `valid` the other way.  (px, py count where (u, v) is inside the
    undistorted image or within eps of its border: elsewhere the pixel is invalid in either arithmetic.)"""
    fw, fh, ss = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["SIZE_SCALE"]
    uw, uh = int(fw * ss), int(fh * ss)
    u, v, px, py, Wd = positions(K, D, H, cfg)
    with np.errstate(invalid="ignore"):
        near = lambda a, *bounds: np.logical_or.reduce([np.abs(a - b) <= eps for b in bounds])
        band_uv = near(u, 0.0, uw - 1.0) | near(v, 0.0, uh - 1.0)
        uv_ok = (Wd != 0) & (u >= -eps) & (u <= uw - 1 + eps) & (v >= -eps) & (v <= uh - 1 + eps)
        band_p = uv_ok & (near(px, -1.0, float(fw)) | near(py, -1.0, float(fh)))
    return band_uv | band_p


def partial_footprints(px, py, valid, fw, fh):
    """bool [BH, BW]: valid pixels whose 2 x 2 footprint has at least one texel outside the frame (BORDER_CONSTANT taps)"""
    sx, sy = np.floor(px), np.floor(py)
    return valid & ((sx < 0) | (sx + 1 > fw - 1) | (sy < 0) | (sy + 1 > fh - 1))


def sample(img, px, py, valid):
    """fp64 bilinear, BORDER_CONSTANT 0 per tap, round half to even -> uint8 [BH, BW, 3]"""
    h, w = img.shape[:2]
    fx, fy = np.floor(px), np.floor(py)
    sx, sy = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = (px - fx)[..., None], (py - fy)[..., None]

    def tap(dx, dy):
        x, y = sx + dx, sy + dy
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        t = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.float64)
        return np.where(ok[..., None], t, 0.0)
    top = (1.0 - ax) * tap(0, 0) + ax * tap(1, 0)
    bot = (1.0 - ax) * tap(0, 1) + ax * tap(1, 1)
    val = np.rint((1.0 - ay) * top + ay * bot)
    return np.where(valid[..., None], np.clip(val, 0, 255), 0).astype(np.uint8)


def gains(image):
    """the (B, G, R) gains oracle.color_balance applies to `image` (surroundBEV.py:43-55), float64"""
    img = np.asarray(image, np.uint8).reshape(-1, 3)
    B, G, R = (float(s) / img.shape[0] for s in img.sum(axis=0, dtype=np.uint64))
    K = (R + G + B) / 3
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([np.float64(K) / np.float64(B), np.float64(K) / np.float64(G), np.float64(K) / np.float64(R)], np.float64)


class AnalyticBevGenerator:
    """BevGenerator(blend, balance)(front, back, left, right, car) with the analytic projection; masks, sums and balance are the
    reference's."""

    def __init__(self, rig, cfg, blend=False, balance=False):
        self.ref = oracle.RefBevGenerator(rig, cfg, blend=blend, balance=False)
        self.balance = bool(balance)
        self.proj = [project(*rig[n], self.ref.cfg) for n in oracle.CAMERAS]

    def with_balance(self, balance):
        """the same generator (projection and masks shared) with balance switched"""
        g = copy.copy(self)
        g.balance = bool(balance)
        return g

    def pre_gain(self, front, back, left, right):
        """the stitched image before color_balance and the car: what the gains are computed from"""
        images = [front, back, left, right]
        if self.balance:
            images = oracle.luminance_balance(images)
        parts = [self.ref.apply_mask(i, sample(img, *self.proj[i])) for i, img in enumerate(images)]
        out = oracle.add_sat(parts[0], parts[1])
        out = oracle.add_sat(out, parts[2])
        return oracle.add_sat(out, parts[3])

    def gains(self, front, back, left, right):
        """the (B, G, R) gains of this frame set (balance generators)"""
        return gains(self.pre_gain(front, back, left, right))

    def __call__(self, front, back, left, right, car=None):
        out = self.pre_gain(front, back, left, right)
        if self.balance:
            out = oracle.color_balance(out)
        if car is not None:
            out = oracle.add_sat(out, car)
        return out
