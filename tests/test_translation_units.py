"""Every kernel of libbevwarp.so is compiled in exactly one translation unit.  bevwarp.hip sees the tile plan only through the
declarations of bevw_planapi.h, and bevwarp_plan.hip does not include bevw_kernels.h: no code object carries a second copy of another
unit's kernels, and no templated kernel is registered from two code objects under one host stub.  Checked on the gfx950 code object of
each unit's object file (no GPU needed)."""
import os

import pytest

from tests._native_build import kernels_of


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    from cameracalibration_amd import build

    build.build()
    tmp = str(tmp_path_factory.mktemp("units"))
    return {u: kernels_of(os.path.join(build.OBJ, u.replace(".hip", ".o")), tmp) for u in build.UNITS}


def test_no_kernel_in_two_units(kernels):
    units = sorted(kernels)
    for i, a in enumerate(units):
        for b in units[i + 1:]:
            assert not kernels[a] & kernels[b], (a, b, sorted(kernels[a] & kernels[b]))


def test_kernels_live_in_their_own_unit(kernels):
    plan_units = {k for k in kernels["bevwarp_plan.hip"] if "k_plan_units" in k}
    assert len(plan_units) == 4, sorted(plan_units)   # k_plan_units<BLEND, SUMS>
    assert any("k_stitch_plan" in k for k in kernels["bevwarp_plan.hip"])
    assert any("k_stitch_pp" in k for k in kernels["bevwarp.hip"])
    assert any("k_jpeg" in k for k in kernels["bevwarp_jpeg.hip"])


def test_instantiation_counts(kernels):
    """The host dispatch picks among a fixed set of kernel instantiations: the legal (input, output, flag) combinations and no others.
    A dispatcher that walks the full product of its flags would multiply them (64 k_stitch_plan kernels instead of 30)."""
    assert {u: len(k) for u, k in kernels.items()} == {"bevwarp.hip": 69, "bevwarp_plan.hip": 54, "bevwarp_jpeg.hip": 24}
    families = {"k_stitch_plan": 30, "k_stitch_pp": 18, "k_remap_lut": 6, "k_vsum": 4, "k_lum_groups": 3, "k_plan_units": 4, "k_units_": 10, "k_shard_pp": 4}
    every = set().union(*kernels.values())
    assert {f: sum(f in k for k in every) for f in families} == families
