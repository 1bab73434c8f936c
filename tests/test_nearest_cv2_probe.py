"""The nearest-neighbour statement (tests/_nearest.py want_nn) against a REAL OpenCV, through tests/golden/nearest_cv2.npz (written by
tests/golden/make_nearest_goldens_with_cv2.py where cv2 exists).  The file does not exist yet -- no cv2 in this image -- so the test skips
and the docs call the rule "unpinned"; the day the file is committed it becomes the pin.  The GPU kernels are held to the statement
(tests/test_nearest_host.py, tests/test_nearest_gpu.py), so this one comparison pins them too."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tests import _nearest as NN

PATH = os.path.join(ROOT, "tests", "golden", "nearest_cv2.npz")


def generator():
    spec = importlib.util.spec_from_file_location("mk_nearest", os.path.join(ROOT, "tests", "golden", "make_nearest_goldens_with_cv2.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


@pytest.mark.skipif(not os.path.exists(PATH), reason="no nearest probe from a real cv2 (tests/golden/make_nearest_goldens_with_cv2.py)")
def test_statement_matches_opencv():
    z = np.load(PATH)
    keys = [str(k) for k in z["keys"]]
    assert len(keys) >= 12 and any(k.startswith("wrap_w") for k in keys) and any(k.startswith("wrap_h") for k in keys)
    for key in keys:
        got = NN.want_nn(z[key + "_src"], z[key + "_map1"], z[key + "_map2"])
        want = z[key + "_dst"]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        assert np.array_equal(got, want), "%s: the statement differs from OpenCV %s in %d pixels" % (key, z["cv2_version"], int((got != want).sum()))


def test_probe_generator_covers_the_wrap_and_the_border():
    """What the generator would hand to cv2, from its seeds alone: both depths of every family, pixels whose nearest texel is inside while
    their footprint is not, and wrap cases in which the unwrapped sum picks another texel; small enough to commit."""
    mk = generator()
    cases = list(mk.cases())
    assert len(cases) == 2 * (len(mk.FAMILIES) + 2) and len({c[0] for c in cases}) == len(cases)
    total = 0
    for key, depth, frame, m1, m2 in cases:
        sh, sw = frame.shape
        assert frame.dtype == NN.DTYPE[depth] and m1.dtype == np.int16 and m2.dtype == np.uint16, key
        total += frame.nbytes // 4 + m1.nbytes + m2.nbytes   # (label frames hold 2 bits per texel: they compress)
        want = NN.want_nn(frame, m1, m2)
        if key.startswith("wrap"):
            unwrapped = NN.want_nn(frame, m1, m2, wrap=False)
            assert (want == 0).any() and unwrapped.all() and not np.array_equal(want, unwrapped), key
        elif key.startswith(("scatter", "corner", "strip")):
            assert (NN.inside_nn(m1, m2, sw, sh) & ~NN.footprint_inside(m1, sw, sh)).any(), key
    assert total < 1_000_000
