"""Which group list a step of the tile plan reads, whether its units may run and what the per-tap kernel is left with, checked WITHOUT a GPU
for every input.

tests/native/plan_route_exhaustive.cpp compiles plan_route and frames_layout (cameracalibration_amd/csrc/bevw_planapi.h) for the host and
holds them against the expressions they replaced -- out_nv12, compact, nv12_units, yuv422_units, use_units, the list chosen, set_stride and
the LUM / SUMS flags, written out there as the specification -- over 4 formats x 2^8 flags x 2^5 existing lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def test_every_route_is_the_one_the_former_expressions_chose(tmp_path):
    from tests import _native_build

    exe = str(tmp_path / "plan_route_exhaustive")
    _native_build.build(os.path.join(ROOT, "tests", "native", "plan_route_exhaustive.cpp"), exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan route ok: %d cases" % (4 * 2 ** 8 * 2 ** 5) in r.stdout, r.stdout
    assert "sampled list ok: %d cases" % (4 * 2) in r.stdout, r.stdout
