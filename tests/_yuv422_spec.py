"""NumPy statement of cv2.cvtColor(img, cv2.COLOR_YUV2BGR_YUY2) and cv2.cvtColor(img, cv2.COLOR_YUV2BGR_UYVY): the specification the packed
4:2:2 input paths of libbevwarp (input_format='yuyv' / 'uyvy') are held to.

The arithmetic is NV12's (tests/_nv12_spec.yuv_to_bgr: OpenCV's YUV -> RGB for 8-bit 4:2:0 and 4:2:2 sources, ITU-R BT.601 limited range,
20-bit fixed point); only the layout differs.  Like the NV12 spec it is pinned against a real cv2 only by
tests/golden/yuv422_cv2_probe.npz (tests/golden/make_yuv422_goldens_with_cv2.py); until that file exists it is "unpinned".  Test
infrastructure only: the product converts on the GPU.

Layout: a frame of W x H texels (W even) is a uint8 array (H, W, 2), the array cv2 takes: per row W / 2 texel pairs of 4 bytes,
Y0 U Y1 V ('yuyv') or U Y0 V Y1 ('uyvy').  Texel (x, y) takes Y from its own two bytes, U and V from the pair x // 2 of its own row."""
import numpy as np

from tests import _nv12_spec as N

ORDERS = ("yuyv", "uyvy")


def components(frames: np.ndarray, order: str):
    """Packed frames [..., H, W, 2] -> Y [..., H, W], U [..., H, W // 2], V [..., H, W // 2]."""
    assert order in ORDERS
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.shape[-1] == 2 and f.shape[-2] % 2 == 0
    y, c = (0, 1) if order == "yuyv" else (1, 0)
    return f[..., y], f[..., 0::2, c], f[..., 1::2, c]


def yuv422_to_bgr(frames: np.ndarray, order: str) -> np.ndarray:
    """Packed frame(s) [..., H, W, 2] -> BGR [..., H, W, 3]: chroma replicated over each horizontal texel pair."""
    Y, U, V = components(frames, order)
    return N.yuv_to_bgr(Y, np.repeat(U, 2, axis=-1), np.repeat(V, 2, axis=-1))


def random_yuv422(rng: np.random.Generator, shape_prefix, width: int, height: int) -> np.ndarray:
    """Uniformly random packed frames [*shape_prefix, height, width, 2] (every byte value in every position, whatever the order)."""
    return rng.integers(0, 256, size=tuple(shape_prefix) + (height, width, 2), dtype=np.uint8)


def bgr_to_yuv422(img: np.ndarray, order: str) -> np.ndarray:
    """BGR [..., H, W, 3] -> packed [..., H, W, 2] (BT.601 limited range, chroma averaged over each texel pair).  Input generation only:
    nothing is compared with this direction."""
    assert order in ORDERS
    f = np.asarray(img).astype(np.float64)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = 16 + 0.257 * R + 0.504 * G + 0.098 * B
    U = 128 - 0.148 * R - 0.291 * G + 0.439 * B
    V = 128 + 0.439 * R - 0.368 * G - 0.071 * B
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    pool = lambda c: 0.5 * (c[..., 0::2] + c[..., 1::2])
    out = np.empty(f.shape[:-1] + (2,), np.uint8)
    y, c = (0, 1) if order == "yuyv" else (1, 0)
    out[..., y] = q(Y)
    out[..., 0::2, c] = q(pool(U))
    out[..., 1::2, c] = q(pool(V))
    return out
