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


# ... and of the one-channel cases: a grey frame set and image of geometry T, a 16-bit frame and image of the far remapper
PLANE_UNIT = {"gray set": 4 * 64 * 48, "gray image": 248 * 250, "gray16 frame": 64 * 48 * 2, "gray16 image": 248 * 250 * 2}


def units():
    return sorted(set(IN_UNIT.values()) | set(OUT_UNIT.values()) | {64 * 48 * 3} | set(PLANE_UNIT.values()))


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


def test_the_literals_of_the_one_channel_and_moving_cases():
    assert PLANE_UNIT == {"gray set": 12288, "gray image": 62000, "gray16 frame": 6144, "gray16 image": 124000}
    assert FB.far_batch(62000) == 69276 > FB.GRID_MAX and [FB.straddler(62000, x) for x in FB.BOUNDARIES] == [34636, 69273]
    assert FB.far_batch(124000) == 34639 and [FB.straddler(124000, x) for x in FB.BOUNDARIES] == [17318, 34636]
    assert 69276 * 12288 < 1 << 31 and 34639 * 6144 < 1 << 31, "the inputs of these cases stay below 2^31: the far side is the output"
    cfg = FB.MOVING_CFG
    in_unit, out_unit = 4 * cfg["FRAME_WIDTH"] * cfg["FRAME_HEIGHT"] * 3, cfg["BEV_WIDTH"] * cfg["BEV_HEIGHT"] * 3
    assert (in_unit, out_unit) == (2304, 3072) and FB.MOVING_BATCH == 65540 > FB.GRID_MAX and FB.MOVING_RIGS == FB.POOL == 7
    assert FB.MOVING_BATCH * in_unit + (FB.MOVING_BATCH + 1) * out_unit + out_unit < 16 << 30, "the child's device allocations"
    for unit in (in_unit, out_unit):
        assert all(x % unit for x in FB.BOUNDARIES)


@pytest.mark.parametrize("batch,in_unit,out_unit", [(69276, 12288, 62000), (65540, 128, 128), (65540, 64, 64), (FB.MOVING_BATCH, 2304, 3072)],
                         ids=["T gray", "gray16 count", "nn8 count", "moving"])
def test_the_sampled_set_contains_the_cut_of_a_grid_of_images(batch, in_unit, out_unit):
    """images 65534 .. 65536 around the first image of the second span (for_each_chunk cuts at 65535), with the ends and every straddler"""
    stride = FB.stride_for(batch)
    why = FB.checked(batch, in_unit, out_unit, stride, range(FB.GRID_MAX - 2, FB.GRID_MAX + 3))
    assert {FB.GRID_MAX - 1, FB.GRID_MAX, FB.GRID_MAX + 1, 0, 1, batch - 2, batch - 1} <= set(why) and "cut of a grid" in why[FB.GRID_MAX]
    for unit in (in_unit, out_unit):
        for boundary in FB.BOUNDARIES:
            s = FB.straddler(unit, boundary)
            if s is not None and s + 1 < batch:
                assert {s - 1, s, s + 1} <= set(why)
    assert math.gcd(stride, 7) == 1 and math.gcd(stride, 16) == 1 and len(why) <= 2300


def test_strides_are_coprime_to_7_and_16():
    for unit in units():
        batch = FB.far_batch(unit)
        s = FB.stride_for(batch)
        assert math.gcd(s, 7) == 1 and math.gcd(s, 16) == 1 and batch // s <= 2200, (batch, s)


def test_case_list():
    cs = FB.cases()
    assert len({c.name for c in cs}) == len(cs) == 17
    assert [c.name for c in cs[:10]] == ["F bgr->bgr plan direct", "F bgr->bgr plan balance", "F nv12->bgr plan direct", "T bgr->bgr plan direct",
                                         "T bgr->bgr plan balance", "T bgr->bgr per_pixel direct", "T bgr->bgr per_pixel balance", "T bgr->nv12 plan direct",
                                         "remap far output", "remap 65540 images"], "the first catalogue is still there, whole"
    assert {(c.name, c.kind, c.schedule, c.depth, c.nearest, bool(c.env)) for c in cs[10:]} == {
        ("T gray->gray plan", "stitch_gray", "plan", 8, False, False), ("T gray->gray per_pixel", "stitch_gray", "per_pixel", 8, False, False),
        ("remap gray16 far output", "plane", None, 16, False, False), ("remap nn16 far output", "plane", None, 16, True, False),
        ("remap gray16 65540 images", "plane_count", None, 16, False, True), ("remap nn8 65540 images", "plane_count", None, 8, True, True),
        ("moving 65540 sets", "moving", None, 8, False, False)}
    assert all(c.env == {"BEVW_REMAP_PLAN": "0"} for c in cs if c.kind == "plane_count")
    got = {(c.geometry, c.inp, c.out, c.schedule, c.mode) for c in cs if c.kind == "stitch"}
    assert got == {("F", "bgr", "bgr", "plan", "direct"), ("F", "bgr", "bgr", "plan", "balance"), ("F", "nv12", "bgr", "plan", "direct"),
                   ("T", "bgr", "bgr", "plan", "direct"), ("T", "bgr", "bgr", "plan", "balance"), ("T", "bgr", "bgr", "per_pixel", "direct"),
                   ("T", "bgr", "bgr", "per_pixel", "balance"), ("T", "bgr", "nv12", "plan", "direct")}
    assert FB.MODES == {"direct": (False, False), "balance": (True, True)} and FB.POOL == 7
    assert [c.env for c in cs if c.kind == "remap_count"] == [{"BEVW_REMAP_PLAN": "0"}] and all(not c.env for c in cs if c.kind not in ("remap_count", "plane_count"))
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
