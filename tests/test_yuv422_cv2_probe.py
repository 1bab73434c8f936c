"""The packed 4:2:2 conversion spec (tests/_yuv422_spec.py) against a REAL OpenCV, through tests/golden/yuv422_cv2_probe.npz (written by
tests/golden/make_yuv422_goldens_with_cv2.py where cv2 exists).  The file does not exist yet, so the comparison skips and the docs call
the conversion "unpinned"; the day the file is committed it becomes the pin.  BEVW_REQUIRE_GOLDENS=1 turns the skip into a failure.  The
GPU kernels are held to the spec (tests/test_yuv422_host.py, tests/test_yuv422_gpu.py), so this one comparison pins them too."""
import os

import numpy as np
import pytest

from conftest import ROOT
from tests import _yuv422_spec as S

PATH = os.path.join(ROOT, "tests", "golden", "yuv422_cv2_probe.npz")
REQUIRE = os.environ.get("BEVW_REQUIRE_GOLDENS", "0") not in ("", "0")


@pytest.mark.skipif(not os.path.exists(PATH) and not REQUIRE, reason="no 4:2:2 probe from a real cv2 (tests/golden/make_yuv422_goldens_with_cv2.py)")
@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("case", ["corners", "random"])
def test_spec_matches_opencv(case, order):
    if not os.path.exists(PATH):
        pytest.fail("BEVW_REQUIRE_GOLDENS is set and %s does not exist" % PATH)
    z = np.load(PATH)
    got = S.yuv422_to_bgr(z[case + "_yuv422"], order)
    want = z[case + "_bgr_" + order]
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max()) == 0, "spec differs from OpenCV %s in %d bytes" % (z["cv2_version"], int(np.count_nonzero(d)))


def test_probe_generator_covers_every_y_against_every_chroma_corner():
    import importlib.util

    spec = importlib.util.spec_from_file_location("mk422", os.path.join(ROOT, "tests", "golden", "make_yuv422_goldens_with_cv2.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    f = mk.corner_frame()
    n = len(mk.CORNERS) ** 2
    assert f.shape == (n, 256, 2) and f.nbytes < 100_000
    Y, U, V = S.components(f, "yuyv")
    for j in range(n):
        assert Y[j].tolist() == list(range(256))
        assert len(set(U[j].tolist())) == 1 and len(set(V[j].tolist())) == 1
    assert {(int(U[j, 0]), int(V[j, 0])) for j in range(n)} == {(u, v) for u in mk.CORNERS for v in mk.CORNERS}
