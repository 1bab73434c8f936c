"""The NV12 conversion spec (tests/_nv12_spec.py) against a REAL OpenCV, through tests/golden/nv12_cv2_probe.npz (written by
tests/golden/make_nv12_goldens_with_cv2.py where cv2 exists).  The file does not exist yet -- no cv2 in this image -- so the test skips and
the docs call the conversion "unpinned"; the day the file is committed it becomes the pin.  The GPU kernels are held to the spec
(tests/test_nv12_host.py, tests/test_nv12_gpu.py), so this one comparison pins them too."""
import os

import numpy as np
import pytest

from conftest import ROOT
from tests import _nv12_spec as S

PATH = os.path.join(ROOT, "tests", "golden", "nv12_cv2_probe.npz")


@pytest.mark.skipif(not os.path.exists(PATH), reason="no NV12 probe from a real cv2 (tests/golden/make_nv12_goldens_with_cv2.py)")
@pytest.mark.parametrize("case", ["corners", "random"])
def test_spec_matches_opencv(case):
    z = np.load(PATH)
    got = S.nv12_to_bgr(z[case + "_nv12"])
    want = z[case + "_bgr"]
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max()) == 0, "spec differs from OpenCV %s in %d bytes" % (z["cv2_version"], int(np.count_nonzero(d)))


def test_probe_generator_covers_every_y_against_every_chroma_corner():
    import importlib.util

    spec = importlib.util.spec_from_file_location("mk", os.path.join(ROOT, "tests", "golden", "make_nv12_goldens_with_cv2.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    f = mk.corner_frame()
    Y, U, V = S.planes(f)
    n = len(mk.CORNERS) ** 2
    assert f.shape == (2 * n * 3 // 2, 128) and f.nbytes < 100_000
    for j in range(n):
        assert sorted(Y[2 * j:2 * j + 2].ravel().tolist()) == list(range(256))
        assert len(set(U[j].tolist())) == 1 and len(set(V[j].tolist())) == 1
    assert {(int(U[j, 0]), int(V[j, 0])) for j in range(n)} == {(u, v) for u in mk.CORNERS for v in mk.CORNERS}
