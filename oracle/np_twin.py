"""Second, independent (vectorised NumPy) statement of the oracle's numeric primitives.  TEST INFRASTRUCTURE ONLY.

Purpose: catch transcription slips in oracle/bevoracle.c.  Both follow SURVEY.md Appendix A; neither is pinned to a
real cv2 (PARITY UNPINNED).  Written array-at-a-time so the code shape shares nothing with the C loops.
"""
from __future__ import annotations

import numpy as np

Q = 32


def _rne(a):
    return np.rint(a)  # round-half-to-even, like cvRound


def fisheye_map(K, D, Knew, size):
    """A.1: fp64 projection per undistorted pixel, Q5 split (surroundBEV.py:98-103)."""
    w, h = size
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k = np.asarray(D, np.float64).reshape(-1)
    ifx, ify = 1.0 / Knew[0, 0], 1.0 / Knew[1, 1]
    x0, y0 = -Knew[0, 2] / Knew[0, 0], -Knew[1, 2] / Knew[1, 1]
    rows = np.arange(h, dtype=np.float64)
    # column walk is an accumulation (+= iR00), reproduced with a sequential ufunc.accumulate
    steps = np.full((h, w), ifx, np.float64)
    steps[:, 0] = rows * 0.0 + x0
    xs = np.add.accumulate(steps, axis=1)
    ys = np.repeat((rows * ify + y0)[:, None], w, axis=1)
    ws = np.repeat((rows * 0.0 + 1.0)[:, None], w, axis=1)
    x, y = xs / ws, ys / ws
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    t4 = t2 * t2
    t6 = t4 * t2
    t8 = t4 * t4
    thd = th * (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.where(r == 0, 1.0, thd / r)
    u = fx * x * scale + cx
    v = fy * y * scale + cy
    iu = _rne(u * Q).astype(np.int64)
    iv = _rne(v * Q).astype(np.int64)
    m1 = np.stack([(iu >> 5), (iv >> 5)], axis=-1).astype(np.int16)
    m2 = ((iv & 31) * Q + (iu & 31)).astype(np.uint16)
    return m1, m2


def pinhole_map(K, D, Knew, size):
    """A.1b: the pinhole ("normal") model, D = k1 k2 p1 p2 k3 [k4 k5 k6] (missing ones 0).  iR = the cofactor inverse of Knew; the column walk
    of _x, _y and _w is an accumulation (+= iR[.., 0]), reproduced with ufunc.accumulate like fisheye_map's.  The (int16) store of iu >> 5 is a
    truncation (a wrap), not a saturation; a non-finite or out-of-range u * 32 rounds to INT_MIN."""
    w, h = size
    fx, fy, u0, v0 = K[0][0], K[1][1], K[0][2], K[1][2]
    d = np.zeros(8, np.float64)
    dv = np.asarray(D, np.float64).reshape(-1)[:8]
    d[:dv.size] = dv
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    iR = invert3x3(Knew)
    rows = np.arange(h, dtype=np.float64)

    def walk(a, b, step):
        steps = np.full((h, w), step, np.float64)
        steps[:, 0] = rows * a + b
        return np.add.accumulate(steps, axis=1)

    _x, _y, _w = walk(iR[0, 1], iR[0, 2], iR[0, 0]), walk(iR[1, 1], iR[1, 2], iR[1, 0]), walk(iR[2, 1], iR[2, 2], iR[2, 0])
    with np.errstate(all="ignore"):
        iw = 1. / _w
        x, y = _x * iw, _y * iw
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2))
        yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy)
        u, v = fx * xd + u0, fy * yd + v0
        iu, iv = _cvround(u * Q), _cvround(v * Q)
    m1 = np.stack([(iu >> 5), (iv >> 5)], axis=-1).astype(np.int16)   # int64 -> int16 keeps the low 16 bits: the wrap of the C cast
    m2 = ((iv & 31) * Q + (iu & 31)).astype(np.uint16)
    return m1, m2


def _cvround(a):
    """cvRound(double) to int32 as cvtsd2si does it: half to even; NaN and everything outside the int32 range give INT_MIN"""
    a = np.asarray(a, np.float64)
    ok = (a > -2147483648.5) & (a < 2147483647.5)
    return np.where(ok, np.rint(np.where(ok, a, 0.0)), float(-2 ** 31)).astype(np.int64)


def invert3x3(m):
    """A.2: cofactor inverse with the documented multiplication order."""
    m = np.asarray(m, np.float64)
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if det == 0.0:
        return np.zeros((3, 3))   # cv::invert of a singular matrix: the result is zero-filled
    s = 1.0 / det
    return np.array([[(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s],
                     [(f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s],
                     [(d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s]])


def perspective_coords(M, dsize, block_width=None):
    """A.2: inverse-map coordinates in Q5, evaluated per column-block origin: blocks of min(1024 / min(16, h), w) columns -- 64 from 16 rows
    on.  block_width: another width, for tests that ask whether a catalogue tells one width from another."""
    w, h = dsize
    bw0 = min(1024 // min(16, h), w) if block_width is None else min(int(block_width), w)
    xs = np.arange(w)
    x0 = (xs // bw0 * bw0).astype(np.float64)[None, :]
    x1 = (xs % bw0).astype(np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    M = np.asarray(M, np.float64).reshape(3, 3)
    X0 = M[0, 0] * x0 + M[0, 1] * y + M[0, 2]
    Y0 = M[1, 0] * x0 + M[1, 1] * y + M[1, 2]
    W0 = M[2, 0] * x0 + M[2, 1] * y + M[2, 2]
    W = W0 + M[2, 0] * x1
    lim = lambda a: np.fmax(float(-2 ** 31), np.fmin(float(2 ** 31 - 1), a))   # fmin / fmax: a NaN gives the other operand, as in C
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        W = np.where(W != 0, Q / W, 0.0)
        X = _rne(lim((X0 + M[0, 0] * x1) * W)).astype(np.int64)
        Y = _rne(lim((Y0 + M[1, 0] * x1) * W)).astype(np.int64)
    xy = np.stack([np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    a = ((Y & 31) * Q + (X & 31)).astype(np.uint16)
    return xy, a


def _taps(src, sx, sy):
    """Fetch the 2x2 neighbourhood with BORDER_CONSTANT 0 per tap."""
    h, w = src.shape[:2]
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = sx + dx, sy + dy
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            t = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            if src.ndim == 3:
                ok = ok[..., None]
            out.append(np.where(ok, t, 0))
    return out


def remap_u8(src, map1, map2):
    """A.4: (sum p*w' + 512) >> 10 with 5-bit-product weights, equal to the Q15 table form for 8-bit data."""
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    code = map2.astype(np.int64) & 1023
    fx, fy = code & 31, code >> 5
    t = [a.astype(np.int64) for a in _taps(src, sx, sy)]
    ws = [(Q - fx) * (Q - fy), fx * (Q - fy), (Q - fx) * fy, fx * fy]
    if src.ndim == 3:
        ws = [x[..., None] for x in ws]
    acc = t[0] * ws[0] + t[1] * ws[1] + t[2] * ws[2] + t[3] * ws[3]
    return ((acc + 512) >> 10).astype(np.uint8)


def remap_f32(src, map1, map2):
    """A.3: float32 weights, float32 left-to-right accumulation, round-half-even, saturate to the source type."""
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    code = map2.astype(np.int64) & 1023
    fx = (code & 31).astype(np.float32) * np.float32(1 / 32)
    fy = (code >> 5).astype(np.float32) * np.float32(1 / 32)
    one = np.float32(1)
    ws = [(one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx]
    t = [a.astype(np.float32) for a in _taps(src, sx, sy)]
    if src.ndim == 3:
        ws = [x[..., None] for x in ws]
    acc = ((t[0] * ws[0] + t[1] * ws[1]) + t[2] * ws[2]) + t[3] * ws[3]
    info = np.iinfo(src.dtype)
    return np.clip(np.rint(acc), info.min, info.max).astype(src.dtype)


def warp_f32(src, M, mode, dsize):
    """A.4b: the float32 family of warpPerspective for the members WITHOUT a fused operation -- every odd `mode` without bit 2 (fma in the
    source position) and bit 4 (fma in the interpolation): 1, 9, 17, 25, 33, 41, 49, 57.  A fused multiply-add rounds once where NumPy's
    float32 arithmetic rounds twice, so the other members have no exact NumPy statement; they are refused here, not approximated.
    M is the INVERSE homography (3 x 3, double); src uint8 or uint16, [h, w] or [h, w, cn]."""
    if not mode & 1 or mode & (2 | 4) or not 0 < mode < 64:
        raise ValueError("warp_f32: member %d contains a fused operation (or is not a member): no exact NumPy statement" % mode)
    f = np.float32
    w, h = dsize
    sh, sw = src.shape[:2]
    M = np.asarray(M, np.float64).reshape(9)
    xi, yi = np.meshgrid(np.arange(w), np.arange(h))
    with np.errstate(all="ignore"):
        if mode & 16:
            xd, yd = xi.astype(np.float64), yi.astype(np.float64)
            den = M[6] * xd + M[7] * yd + M[8]
            px = ((M[0] * xd + M[1] * yd + M[2]) / den).astype(f)
            py = ((M[3] * xd + M[4] * yd + M[5]) / den).astype(f)
        else:
            m, fx, fy = M.astype(f), xi.astype(f), yi.astype(f)
            num_x, num_y, den = (fx * m[0] + fy * m[1]) + m[2], (fx * m[3] + fy * m[4]) + m[5], (fx * m[6] + fy * m[7]) + m[8]
            if mode & 32:
                inv = f(1) / den
                px, py = num_x * inv, num_y * inv
            else:
                px, py = num_x / den, num_y / den
        assert px.dtype == f and py.dtype == f
        live = (px > f(-2)) & (px < f(sw) + f(1)) & (py > f(-2)) & (py < f(sh) + f(1))
        px, py = np.where(live, px, f(0)), np.where(live, py, f(0))
        bx, by = np.floor(px), np.floor(py)
        tx, ty = px - bx, py - by
        t = [a.astype(f) for a in _taps(src, bx.astype(np.int64), by.astype(np.int64))]
        if src.ndim == 3:
            tx, ty, live = tx[..., None], ty[..., None], live[..., None]

        def mix(lo, hi, u):
            if mode & 8:
                return (f(1) - u) * lo + u * hi
            return lo + u * (hi - lo)

        acc = mix(mix(t[0], t[1], tx), mix(t[2], t[3], tx), ty)
        assert acc.dtype == f
    info = np.iinfo(src.dtype)
    return np.where(live, np.clip(np.rint(acc), info.min, info.max), 0).astype(src.dtype)


def translate(img, shift_x, shift_y):
    """CenterImage.translate: dst(x, y) = src(x - shift_x, y - shift_y), 0 outside -- a slice of the image laid into zeros."""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    sx, sy = int(shift_x), int(shift_y)
    if abs(sx) < w and abs(sy) < h:
        out[max(sy, 0):h + min(sy, 0), max(sx, 0):w + min(sx, 0)] = img[max(-sy, 0):h - max(sy, 0), max(-sx, 0):w - max(sx, 0)]
    return out


def resize_dsize(w, h, fx, fy):
    """(cvRound(w fx), cvRound(h fy)): half to even"""
    return int(np.rint(np.float64(w) * np.float64(fx))), int(np.rint(np.float64(h) * np.float64(fy)))


def _resize_axis(n_src, n_dst, scale, clamp_frac):
    """source index and the two 11-bit weights per destination index: the position in float32, floorf, the fraction in float32"""
    f = np.float32
    pos = ((np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(scale) - 0.5).astype(f)
    s = np.floor(pos)
    frac = pos - s
    s = s.astype(np.int64)
    if clamp_frac:   # columns: a tap pair that leaves the image takes the edge texel whole
        frac = np.where((s < 0) | (s >= n_src - 1), f(0), frac)
        s = np.where(s < 0, 0, np.where(s >= n_src - 1, n_src - 1, s))
    c0 = np.rint((f(1) - frac) * f(2048)).astype(np.int64)
    c1 = np.rint(frac * f(2048)).astype(np.int64)
    return s, c0, c1


def resize_linear(img, fx, fy):
    """cv2.resize(img, (0, 0), fx, fy), INTER_LINEAR, 8UC3: scale = 1 / f, 11-bit weights, the horizontal pass in int32 and the vertical pass
    of the 8U specialisation, (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2; rows clip the tap pair into the image."""
    h, w = img.shape[:2]
    dw, dh = resize_dsize(w, h, fx, fy)
    xs, a0, a1 = _resize_axis(w, dw, 1.0 / np.float64(fx), True)
    ys, b0, b1 = _resize_axis(h, dh, 1.0 / np.float64(fy), False)
    x1 = np.minimum(xs + 1, w - 1)
    r0, r1 = np.clip(ys, 0, h - 1), np.clip(ys + 1, 0, h - 1)
    src = img.astype(np.int64)
    hor = src[:, xs] * a0[None, :, None] + src[:, x1] * a1[None, :, None]          # [h, dw, 3]
    S0, S1 = hor[r0], hor[r1]
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def bgr2hsv(img):
    """A.7 forward: integer tables, H in [0, 180)."""
    idx = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(idx > 0, np.rint((255 << 12) / (1.0 * idx)), 0).astype(np.int64)
        hdiv = np.where(idx > 0, np.rint((180 << 12) / (6.0 * idx)), 0).astype(np.int64)
    b, g, r = (img[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([np.clip(h, 0, 255), s, v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv):
    """A.7 inverse: float32 sector formula, *255 and round-half-even."""
    f = np.float32
    h = hsv[..., 0].astype(f) * f(6.0 / 180.0)
    s = hsv[..., 1].astype(f) * f(1.0 / 255.0)
    v = hsv[..., 2].astype(f) * f(1.0 / 255.0)
    h = np.fmod(h, f(6))
    sec = np.floor(h).astype(np.int64)
    frac = h - sec.astype(f)
    bad = (sec < 0) | (sec >= 6)
    sec = np.where(bad, 0, sec)
    frac = np.where(bad, f(0), frac)
    one = f(1)
    tab = np.stack([v, v * (one - s), v * (one - s * frac), v * (one - s * (one - frac))], axis=-1)
    sel = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sec]
    bgr = np.take_along_axis(tab, sel, axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * f(255)), 0, 255).astype(np.uint8)
