"""NumPy statement of the NV12 OUTPUT of libbevwarp (bevw_set_output_format, BevGenerator(output_format='nv12'),
Undistorter(output_format='nv12')): the specification the kernels are held to.

The conversion is cv2.cvtColor(bgr, cv2.COLOR_BGR2YUV_I420) with its U and V planes interleaved (U first), restated from OpenCV's
RGB8toYUV420pInvoker (color_yuv.simd.hpp: ITU-R BT.601 limited range, 20-bit fixed point).  The chroma of the 2 x 2 block (i, j) comes
from its top-left pixel (2j, 2i) ALONE -- OpenCV does not average the block.  It is pinned against a real cv2 only by
tests/golden/nv12_out_cv2_probe.npz (tests/golden/make_nv12_out_goldens_with_cv2.py); until that file exists the arithmetic is "unpinned".
Test infrastructure only: the product converts on the GPU (csrc/bevw_device.h: bgr_to_y, bgr_to_uv, nv12_quad).

Layout: an NV12 image of W x H pixels (both even) is a uint8 array (H * 3 // 2, W): H rows of Y, then H / 2 rows of interleaved U, V.
On the device the rows have `pitch` bytes (the handle's output pitch) in both planes."""
import numpy as np

Y_COEF = (269484, 528482, 102760)        # R, G, B
U_COEF = (-155188, -305135, 460324)
V_COEF = (460324, -385875, -74448)
Y_ADD = (16 << 20) + (1 << 19)
C_ADD = (128 << 20) + (1 << 19)


def bgr_to_yuv(img) -> tuple:
    """uint8 [..., 3] (B, G, R) -> Y, U, V uint8 arrays [...] of every pixel (no subsampling)."""
    a = np.asarray(img).astype(np.int64)
    B, G, R = a[..., 0], a[..., 1], a[..., 2]
    f = lambda c, add: (c[0] * R + c[1] * G + c[2] * B + add) >> 20   # arithmetic shift; every sum is positive
    Y, U, V = f(Y_COEF, Y_ADD), f(U_COEF, C_ADD), f(V_COEF, C_ADD)
    assert Y.min(initial=16) >= 16 and Y.max(initial=235) <= 235 and min(U.min(initial=16), V.min(initial=16)) >= 16
    assert max(U.max(initial=240), V.max(initial=240)) <= 240   # no clamp ever applies
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def bgr_to_nv12(img) -> np.ndarray:
    """BGR [..., H, W, 3] (H, W even) -> NV12 [..., H * 3 // 2, W]: chroma of each 2 x 2 block from its top-left pixel."""
    img = np.asarray(img)
    H, W = img.shape[-3], img.shape[-2]
    assert H % 2 == 0 and W % 2 == 0, "NV12 needs even sizes"
    Y, U, V = bgr_to_yuv(img)
    UV = np.empty(Y.shape[:-2] + (H // 2, W), np.uint8)
    UV[..., 0::2] = U[..., 0::2, 0::2]
    UV[..., 1::2] = V[..., 0::2, 0::2]
    return np.concatenate([Y, UV], axis=-2)


def planes(nv12: np.ndarray):
    """NV12 image(s) [..., H * 3 // 2, W] -> Y [..., H, W], UV [..., H // 2, W] (interleaved U, V)."""
    nv12 = np.asarray(nv12)
    H = nv12.shape[-2] * 2 // 3
    return nv12[..., :H, :], nv12[..., H:, :]


def from_device(buf: np.ndarray, bw: int, bh: int, pitch: int, index: int = 0) -> np.ndarray:
    """Image `index` of a device buffer of NV12 images with rows of `pitch` bytes (flat uint8) -> dense [bh * 3 // 2, bw]: the Y plane at
    byte index * pitch * bh * 3 // 2, the U / V plane bh * pitch bytes after it."""
    img = np.asarray(buf).reshape(-1)[index * pitch * bh * 3 // 2:(index + 1) * pitch * bh * 3 // 2]
    return img.reshape(bh * 3 // 2, pitch)[:, :bw]
