"""The format dispatch of the host code on the branches only an environment switch reaches:

  BEVW_BAL_MODE=0     balance as the luminance round trip per tap: k_stitch_plan<BLEND, LUM, SUMS, kLayoutNV12 | kLayoutSurf, ..>
  BEVW_PLAN_UNITS=0   the plan's per-tap kernel over every tile, no unit kernel
  BEVW_REMAP_PLAN=0   remap_launch (k_remap_lut) on an aligned remapper that would otherwise run its plan; the per-pixel stitch is untouched

The library reads the switches once per process, so each runs in a fresh child (tests/_format_dispatch_worker.py), one after the other,
each under its own timeout; the first child that does not exit 0 ends the test.  Every child runs the small rig of tests/_harness.py
(320 x 256 frames, 248 x 250 BEV, batch 3) over packed BGR, packed NV12 and NV12 surfaces at pitch FW + 4, BGR and NV12 images, all four
(blend, balance) modes, each with a car; the BEVW_REMAP_PLAN=0 child also the fisheye undistorter at batch 3.  Expected values: the CPU
oracle on the _nv12_spec-converted frames (through _nv12_out_spec for NV12 images), computed once here and shared through a file;
tolerance 0, pixels no camera covers included.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from tests import _nv12_spec as S
from tests import _harness as H

pytestmark = pytest.mark.gpu

SWITCHES = ("BEVW_BAL_MODE", "BEVW_PLAN_UNITS", "BEVW_REMAP_PLAN")
MODES = ((0, 0), (1, 0), (0, 1), (1, 1))   # (blend, balance), as in the worker
CHILD_TIMEOUT = 180   # seconds: a library load, 24 small handles (+ 6 remappers) and their steps take a few seconds


@pytest.fixture(scope="module")
def case_file(oracle, tmp_path_factory):
    cfg = H.SMALL_CFG
    fw, fh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"]
    rng = np.random.default_rng(4100)
    nv = S.random_nv12(rng, (3, 4), fw, fh)
    bgr = np.stack([np.stack(S.nv12_to_bgr(nv[b])) for b in range(3)])
    car = H.random_car(rng, cfg)
    z = dict(nv=nv, bgr=bgr, car=car)
    for m, (blend, balance) in enumerate(MODES):
        ref = oracle.RefBevGenerator(H.small_rig(), cfg, blend=bool(blend), balance=bool(balance))
        z["none%d" % m] = H.uncovered(ref)
        assert z["none%d" % m].any()
        z["want%d" % m] = np.stack([ref(*bgr[b], car) for b in range(3)])
    # the fisheye undistorter of the front camera, default scales: the output has the frame's size
    K, D, _ = H.small_rig()["front"]
    o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, oracle.camera_mat_dst(K, fw, fh, 1.0, 1.0), (fw, fh))
    z["und_size"] = np.array([fw, fh])
    z["und_outside"] = (o1[..., 0] < -1) | (o1[..., 0] >= fw) | (o1[..., 1] < -1) | (o1[..., 1] >= fh)
    z["und_want"] = np.stack([oracle.remap(bgr[b, 0], o1, o2) for b in range(3)])
    path = str(tmp_path_factory.mktemp("format_dispatch") / "case.npz")
    np.savez(path, **z)
    return path


def test_switched_branches_match_oracle(case_file):
    for switch in SWITCHES:
        H.run_child("_format_dispatch_worker.py", [case_file, switch], {switch: "0"}, SWITCHES, CHILD_TIMEOUT, "worker OK " + switch)
