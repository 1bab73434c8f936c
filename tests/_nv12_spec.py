"""NumPy statement of cv2.cvtColor(img, cv2.COLOR_YUV2BGR_NV12): the specification the NV12 input paths of libbevwarp are held to.

Restated from OpenCV's YUV420sp -> RGB conversion (color_yuv.simd.hpp: ITU-R BT.601 limited range, 20-bit fixed point).  It is pinned
against a real cv2 only by tests/golden/nv12_cv2_probe.npz (tests/golden/make_nv12_goldens_with_cv2.py); until that file exists the
arithmetic is "unpinned".  Test infrastructure only: the product converts on the GPU (csrc/bevw_device.h: nv12_bgr).

Layout: an NV12 frame of W x H texels (both even) is a uint8 array (H * 3 // 2, W): H rows of Y, then H / 2 rows of interleaved U, V
(U first).  Texel (x, y) takes Y[y, x], U = UV[y // 2, 2 * (x // 2)], V = UV[y // 2, 2 * (x // 2) + 1]."""
import numpy as np


def yuv_to_bgr(Y, U, V) -> np.ndarray:
    """uint8 arrays (broadcast together) -> uint8 [..., 3] (B, G, R)."""
    Y, U, V = np.broadcast_arrays(*(np.asarray(a).astype(np.int64) for a in (Y, U, V)))
    uu, vv = U - 128, V - 128
    ruv = (1 << 19) + 1673527 * vv
    guv = (1 << 19) - 852492 * vv - 409993 * uu
    buv = (1 << 19) + 2116026 * uu
    yy = np.maximum(0, Y - 16) * 1220542
    out = [np.clip((yy + c) >> 20, 0, 255) for c in (buv, guv, ruv)]   # arithmetic shift
    return np.stack(out, axis=-1).astype(np.uint8)


def planes(frame: np.ndarray):
    """NV12 frame (H * 3 // 2, W) -> Y (H, W), U (H // 2, W // 2), V (H // 2, W // 2)."""
    frame = np.asarray(frame)
    H = frame.shape[-2] * 2 // 3
    Y = frame[..., :H, :]
    UV = frame[..., H:, :]
    return Y, UV[..., 0::2], UV[..., 1::2]


def nv12_to_bgr(frame: np.ndarray) -> np.ndarray:
    """NV12 frame(s) [..., H * 3 // 2, W] -> BGR [..., H, W, 3]: chroma replicated over each 2 x 2 block."""
    Y, U, V = planes(frame)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)
    return yuv_to_bgr(Y, up(U), up(V))


def bgr_to_nv12(img: np.ndarray) -> np.ndarray:
    """BGR [..., H, W, 3] -> NV12 [..., H * 3 // 2, W] (BT.601 limited range, chroma averaged over 2 x 2 blocks).  Input generation only:
    nothing is compared with this direction."""
    f = np.asarray(img).astype(np.float64)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = 16 + 0.257 * R + 0.504 * G + 0.098 * B
    U = 128 - 0.148 * R - 0.291 * G + 0.439 * B
    V = 128 + 0.439 * R - 0.368 * G - 0.071 * B
    pool = lambda c: 0.25 * (c[..., 0::2, 0::2] + c[..., 1::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 1::2])
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    U, V = q(pool(U)), q(pool(V))
    UV = np.empty(U.shape[:-1] + (U.shape[-1] * 2,), np.uint8)
    UV[..., 0::2], UV[..., 1::2] = U, V
    return np.concatenate([q(Y), UV], axis=-2)


def random_nv12(rng: np.random.Generator, shape_prefix, width: int, height: int) -> np.ndarray:
    """Uniformly random NV12 frames [*shape_prefix, height * 3 // 2, width]."""
    return rng.integers(0, 256, size=tuple(shape_prefix) + (height * 3 // 2, width), dtype=np.uint8)
