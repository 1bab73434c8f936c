"""The NV12 output spec (tests/_nv12_out_spec.py) against a REAL OpenCV, through tests/golden/nv12_out_cv2_probe.npz (written by
tests/golden/make_nv12_out_goldens_with_cv2.py where cv2 exists).  The file does not exist yet -- no cv2 in this image -- so the comparison
skips and the docs call the conversion "unpinned"; the day the file is committed it becomes the pin.  The kernels are held to the spec
(tests/test_nv12_out_host.py, tests/test_nv12_out_gpu.py), so this one comparison pins them too."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tests import _nv12_out_spec as S

PATH = os.path.join(ROOT, "tests", "golden", "nv12_out_cv2_probe.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("mk", os.path.join(ROOT, "tests", "golden", "make_nv12_out_goldens_with_cv2.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def i420_to_nv12(i420: np.ndarray) -> np.ndarray:
    """cv2's I420 (H * 3 // 2, W): Y, then the U plane and the V plane of (H / 2) x (W / 2) each, row-major -> NV12 (U / V interleaved)."""
    H, W = i420.shape[0] * 2 // 3, i420.shape[1]
    flat = i420.reshape(-1)
    U = flat[H * W:H * W + H * W // 4].reshape(H // 2, W // 2)
    V = flat[H * W + H * W // 4:].reshape(H // 2, W // 2)
    UV = np.empty((H // 2, W), np.uint8)
    UV[:, 0::2], UV[:, 1::2] = U, V
    return np.concatenate([i420[:H], UV])


@pytest.mark.skipif(not os.path.exists(PATH), reason="no NV12 output probe from a real cv2 (tests/golden/make_nv12_out_goldens_with_cv2.py)")
@pytest.mark.parametrize("case", ["blocks", "ramps"])
def test_spec_matches_opencv(case):
    z = np.load(PATH)
    want = i420_to_nv12(z[case + "_i420"])
    got = S.bgr_to_nv12(z[case + "_bgr"])
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max()) == 0, "spec differs from OpenCV %s in %d bytes" % (z["cv2_version"], int(np.count_nonzero(d)))


def test_i420_layout_helper():
    i420 = np.arange(6 * 4, dtype=np.uint8).reshape(6, 4)   # 4 x 4 image: 16 Y, 4 U, 4 V
    nv = i420_to_nv12(i420)
    assert nv[:4].tolist() == i420[:4].tolist()
    assert nv[4].tolist() == [16, 20, 17, 21] and nv[5].tolist() == [18, 22, 19, 23]


def test_probe_tells_top_left_from_averaged_chroma_and_pins_rounding():
    """Without cv2: the probe's inputs can tell the two chroma rules apart, and reach every value of every channel."""
    mk = _generator()
    img = mk.blocks_image()
    assert img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0 and img.nbytes < 50_000
    _, U, V = S.bgr_to_yuv(img)
    block_mean = lambda c: c.astype(np.float64).reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
    tl = np.stack([U[0::2, 0::2], V[0::2, 0::2]]).astype(np.float64)
    avg = np.stack([block_mean(U), block_mean(V)])   # the chroma an averaging converter would store (up to its rounding)
    differ = np.mean(np.any(np.abs(tl - avg) >= 2, axis=0))
    assert differ > 0.9, "the probe's blocks would not tell top-left chroma from averaged chroma (%.2f)" % differ
    r = mk.ramps_image()
    assert (r[0::2] == r[1::2]).all() and (r[:, 0::2] == r[:, 1::2]).all()   # one colour per 2 x 2 block: nothing to average
    for ch in range(3):
        assert set(r[..., ch].ravel().tolist()) == set(range(256))
    # the fixed-point fractions reach both sides of every rounding boundary: some Y, U and V within 1 / 64 of .5 above and below
    rb = r[0::2, 0::2].reshape(-1, 3).astype(np.int64)
    for coef, add in ((S.Y_COEF, S.Y_ADD), (S.U_COEF, S.C_ADD), (S.V_COEF, S.C_ADD)):
        frac = ((coef[0] * rb[:, 2] + coef[1] * rb[:, 1] + coef[2] * rb[:, 0] + add - (1 << 19)) % (1 << 20)) / 2 ** 20
        assert ((frac > 0.5 - 1 / 64) & (frac < 0.5)).any() and ((frac >= 0.5) & (frac < 0.5 + 1 / 64)).any()
