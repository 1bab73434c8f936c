"""The host leg of the far batches (tests/_far_batches.py) -- WITHOUT a GPU: the index arithmetic the worker derives its batches and straddlers
with, on plain integers; the case list; and the geometry T (64 x 48 frames -> 248 x 250 BEV), which exists only to make a long batch cheap
and must still be a stitch worth comparing: every camera covers its share, cameras overlap, pixels stay uncovered, outputs are not black."""
import math

import numpy as np
import pytest

from tests import _far_batches as FB
from tests._harness import uncovered

# bytes per frame set / per image of the cases: (geometry, input format) and (geometry, output format)
IN_UNIT = {("F", "bgr"): 4 * 320 * 256 * 3, ("F", "nv12"): 4 * 320 * 256 * 3 // 2, ("T", "bgr"): 4 * 64 * 48 * 3}
OUT_UNIT = {"bgr": 248 * 250 * 3, "nv12": 248 * 250 * 3 // 2}


def units():
    return sorted(set(IN_UNIT.values()) | set(OUT_UNIT.values()) | {64 * 48 * 3})


@pytest.mark.parametrize("boundary", FB.BOUNDARIES)
@pytest.mark.parametrize("unit", units())
def test_exactly_one_unit_straddles_a_boundary_and_the_batch_reaches_two_units_past_it(unit, boundary):
    assert boundary % unit != 0, "a unit ends exactly on the boundary: nothing straddles it"
    batch = FB.far_batch(unit)
    hits = [b for b in range(max(0, boundary // unit - 4), boundary // unit + 5) if b * unit < boundary < (b + 1) * unit]
    assert hits == [FB.straddler(unit, boundary)]
    s = hits[0]
    assert (s - 1 + 1) * unit <= boundary and (s + 1) * unit > boundary          # (no unit before s reaches it, none after s starts below it)
    assert s + 2 <= batch - 1 and batch * unit > boundary + 2 * unit
    why = FB.checked(batch, unit, unit, FB.stride_for(batch))
    assert {s - 1, s, s + 1, 0, 1, batch - 2, batch - 1} <= set(why) and "straddles 2^%d" % (boundary.bit_length() - 1) in why[s]
    assert max(why) == batch - 1 and min(why) == 0


def test_the_literals_of_the_two_geometries():
    assert IN_UNIT[("F", "bgr")] == 983040 and FB.far_batch(983040) == 4372 and [FB.straddler(983040, x) for x in FB.BOUNDARIES] == [2184, 4369]
    assert IN_UNIT[("T", "bgr")] == 36864 and OUT_UNIT["bgr"] == 186000 and FB.far_batch(186000) == 23094
    assert [FB.straddler(186000, x) for x in FB.BOUNDARIES] == [11545, 23091]
    frames = 23094 * 4
    assert frames == 92376 > FB.GRID_MAX and FB.GRID_MAX // 4 == 16383 and FB.GRID_MAX % 4 == 3, "the first cut of k_vsum: set 16383, camera 3"
    assert set(FB.VSUM_CUT) == {16382, 16383, 16384, 16385}
    # the plan schedule slices a balance batch in two: neither slice's frames reach the cut (the driver's docstring says so)
    assert frames // 2 < FB.GRID_MAX
    assert FB.COUNT_BATCH == 65540 > FB.GRID_MAX


def test_strides_are_coprime_to_7_and_16():
    for unit in units():
        batch = FB.far_batch(unit)
        s = FB.stride_for(batch)
        assert math.gcd(s, 7) == 1 and math.gcd(s, 16) == 1 and batch // s <= 2200, (batch, s)


def test_case_list():
    cs = FB.cases()
    assert len({c.name for c in cs}) == len(cs) == 10
    got = {(c.geometry, c.inp, c.out, c.schedule, c.mode) for c in cs if c.kind == "stitch"}
    assert got == {("F", "bgr", "bgr", "plan", "direct"), ("F", "bgr", "bgr", "plan", "balance"), ("F", "nv12", "bgr", "plan", "direct"),
                   ("T", "bgr", "bgr", "plan", "direct"), ("T", "bgr", "bgr", "plan", "balance"), ("T", "bgr", "bgr", "per_pixel", "direct"),
                   ("T", "bgr", "bgr", "per_pixel", "balance"), ("T", "bgr", "nv12", "plan", "direct")}
    assert FB.MODES == {"direct": (False, False), "balance": (True, True)} and FB.POOL == 7
    assert [c.env for c in cs if c.kind == "remap_count"] == [{"BEVW_REMAP_PLAN": "0"}] and all(not c.env for c in cs if c.kind != "remap_count")
    assert FB.GEOMETRIES["F"][1] == "in" and FB.GEOMETRIES["T"][1] == "out"


def test_geometry_t_is_not_degenerate(oracle):
    cfg = FB.CFG_T
    rig = FB.scaled_rig(cfg)
    direct, blend = oracle.RefBevGenerator(rig, cfg, blend=False), oracle.RefBevGenerator(rig, cfg, blend=True)
    cover = [float((np.asarray(m) != 0).mean()) for m in direct.masks]
    two = lambda ref: int((np.sum([np.asarray(m) != 0 for m in ref.masks], axis=0) == 2).sum())
    none = int(uncovered(direct).sum())
    _, back, car = FB.pool(cfg, "bgr")
    img = direct(*back[0], car)
    inside = float(img[~uncovered(direct)].any(-1).mean())
    print("T: cover %s, two contributors %d direct %d blend, uncovered %d, non-zero share of covered pixels %.3f" % (
        ["%.2f" % c for c in cover], two(direct), two(blend), none, inside))
    assert min(cover) >= 0.15 and two(direct) >= 400 and two(blend) >= 10000 and none >= 5000
    assert inside >= 0.85, "most covered pixels sample a texel inside the 64 x 48 frames"


@pytest.mark.parametrize("geometry,inp", sorted(IN_UNIT))
def test_pool_sets_differ_in_brightness(geometry, inp):
    cfg, _ = FB.GEOMETRIES[geometry]
    native, back, car = FB.pool(cfg, inp)
    assert native.shape[0] == back.shape[0] == FB.POOL and native[0].nbytes == IN_UNIT[(geometry, inp)] and car.any()
    means = back.reshape(FB.POOL, 4, -1).mean(-1)
    assert len({tuple(np.round(m, 1)) for m in means}) == FB.POOL and (np.ptp(means, axis=1) > 10).all(), means
