"""The camera-shard catalogue (tests/_shard_cases.py) on the host: pins the checker of tests/test_shard_cases_gpu.py.  Oracle only.

  * regrouping  the oracle shard engine's parts, combined, equal oracle.RefBevGenerator byte for byte: every geometry x {(direct, no
                balance), (blend, balance)} x partition x frame set, and the rig families at two partitions -- the fact the camera-per-GPU
                design rests on (cv2.add saturates, so min(255, sum) does not depend on the grouping);
  * census      the boxes and the bytes that saturate before the car equal the recorded tables, the floors hold, the synthetic part lists
                hit their classes -- no case passes emptily;
  * statement   the NumPy statement of the combine equals the O.add_sat chain of OracleShardEngine.combine on the synthetic lists;
  * controls    a box shifted by a pixel, a part read with a stride one row off, a wrapping add: the statement tells each from the chain."""
import ast
import os

import numpy as np
import pytest

from tests import _shard_cases as K
from tests import _shard_common as SC
from tests._shard_oracle import OracleShardEngine, mask_box

_shards = {}


def shards(kind, name, blend, balance):
    key = (kind, name, blend, balance)
    if key not in _shards:
        rig, cfg, frames, car = K.subject(kind, name)
        _shards[key] = (K.OracleShards(rig, cfg, frames, blend, balance), rig, cfg, frames, car)
    return _shards[key]


def check_regrouping(oracle, kind, name, blend, balance, partitions):
    s, rig, cfg, frames, car = shards(kind, name, blend, balance)
    ref = oracle.RefBevGenerator(rig, cfg, blend=blend, balance=balance)
    want = np.stack([ref(*fs, car=car) for fs in frames])
    bare = np.stack([ref(*fs) for fs in frames])
    for part in partitions:
        got = s.combine(part, car)
        for b in range(len(frames)):   # geometries: b is the frame set of SC.CONTENT
            assert np.array_equal(got[b], want[b]), "%s %s blend %d balance %d, partition %s, frame set %d: %d bytes differ" % (
                kind, name, blend, balance, part, b, int((got[b] != want[b]).sum()))
        assert np.array_equal(s.combine(part, None), bare), "%s %s, partition %s, no car" % (kind, name, part)
        # the statement on real parts, too
        boxes = [s.engine(c).box for c in part]
        st = K.combine_statement([s.part(c) for c in part], boxes, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], car, balance)
        assert np.array_equal(st, want), "%s %s, partition %s: the NumPy statement differs from the oracle" % (kind, name, part)


def test_partitions_extend_those_of_the_shard_tests():
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_camera_shard.py")).read())
    theirs = [ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "PARTITIONS"]
    assert len(theirs) == 1 and list(K.PARTITIONS[:len(theirs[0])]) == theirs[0]
    assert [(0, 3), (1, 2)] in K.PARTITIONS and [(0, 1, 2), (3,)] in K.PARTITIONS
    for part in K.PARTITIONS + K.RIG_PARTITIONS:
        assert sorted(c for cams in part for c in cams) == [0, 1, 2, 3]


@pytest.mark.parametrize("blend,balance", K.MODES)
@pytest.mark.parametrize("geo", K.GEOMETRIES, ids=K.geo_name)
def test_geometry_parts_regroup_to_the_reference(oracle, geo, blend, balance):
    check_regrouping(oracle, "geo", geo, blend, balance, K.PARTITIONS)


@pytest.mark.parametrize("blend,balance", K.MODES)
@pytest.mark.parametrize("name", K.RIG_FAMILIES)
def test_rig_family_parts_regroup_to_the_reference(oracle, name, blend, balance):
    check_regrouping(oracle, "rig", name, blend, balance, K.RIG_PARTITIONS)


# ---------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", K.GEOMETRIES, ids=K.geo_name)
def test_geometry_census(oracle, geo):
    bw, bh = geo[:2]
    for blend, balance in K.MODES:
        s = shards("geo", geo, blend, balance)[0]
        boxes = [s.engine(c).box for c in K.SINGLES]
        assert boxes == K.BOXES[geo][blend], (geo, blend, boxes)
        for x0, y0, x1, y1 in boxes:
            assert 0 <= x0 < x1 <= bw and 0 <= y0 < y1 <= bh and x0 % 4 == 0 and ((x1 - x0) % 4 == 0 or x1 == bw)
        # a shard of several cameras: the box of the union of their masks
        for part in K.PARTITIONS:
            for cams in part:
                assert s.engine(cams).box == mask_box([s.engine((c,)).masks[c] for c in cams], bw, bh)
        sums = K.part_sums([s.part(c) for c in K.SINGLES], boxes, bw, bh)
        counts = tuple(int((sums[b] > 255).sum()) for b in range(len(SC.CONTENT)))
        print("%s blend %d balance %d: bytes above 255 before the car (%s) = %s" % (K.geo_name(geo), blend, balance, ", ".join(SC.CONTENT), counts))
        assert counts == K.SATURATED[geo][(blend, balance)]
    white = SC.CONTENT.index("white")
    assert K.SATURATED[geo][(False, False)][white] > 0 and K.SATURATED[geo][(False, False)][SC.CONTENT.index("random")] > 0


def test_census_names_the_boxes_the_other_geometries_never_made():
    B = K.BOXES
    assert B[(260, 250, 62, 250)][False][1] == (0, 0, 4, 1) and B[(260, 250, 62, 250)][False][0] == (0, 0, 260, 1)      # empty mask, one row
    assert B[(260, 250, 260, 100)][False][3] == (0, 0, 4, 1) and B[(260, 250, 260, 100)][False][2] == (0, 0, 4, 250)   # empty mask, one column
    assert B[(253, 255, 63, 101)][True][3] == (156, 0, 253, 255) and B[(270, 270, 50, 88)][True][3] == (160, 0, 270, 270)
    assert {g[0] % 4 for g in K.GEOMETRIES} >= {0, 1, 2}
    assert K.SATURATED[(252, 180, 0, 0)][(True, True)][SC.CONTENT.index("white")] > 0
    assert all(K.SATURATED[g][(True, True)] == (0, 0, 0) for g in K.GEOMETRIES if g != (252, 180, 0, 0))   # why that geometry is there


@pytest.mark.parametrize("bw,bh", K.SYNTH_BEVS)
def test_synthetic_lists_hit_their_classes(oracle, bw, bh):
    cases = K.synthetic(bw, bh)
    for name, boxes in cases.items():
        assert 1 <= len(boxes) <= 8, name
        for x0, y0, x1, y1 in boxes:
            assert 0 <= x0 < x1 <= bw and 0 <= y0 < y1 <= bh, (name, (x0, y0, x1, y1))
    hit = K.synthetic_classes(bw, bh)
    for cls in ("x0_unaligned", "width_unaligned", "more_than_4_parts", "depth_3", "saturated"):
        assert hit[cls], "%d x %d: no synthetic case of class %s" % (bw, bh, cls)
    assert {b[0] % 4 for boxes in cases.values() for b in boxes} == {0, 1, 2, 3}
    assert bool(hit["dword_eligible"]) == (bw % 4 == 0)
    if bw % 4 == 0:   # the dword kernel meets overlap, more than 4 parts, parts that start at different rows, and saturation
        assert {"stack8", "overlap_aligned", "build4"} <= set(hit["dword_eligible"]) and "stack8" in hit["saturated"]
    assert any(b == (0, 0, 1, 1) for b in cases["corners_1x1"]) and (bw - 1, bh - 1, bw, bh) in cases["corners_1x1"]
    d = K.depth(cases["disjoint"], bw, bh)
    assert d.max() == 1 and (d == 0).mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------
# the NumPy statement against the oracle engine's add_sat chain, and its negative controls
# ---------------------------------------------------------------------------------------------------------------
def chain_engine(bw, bh, balance):
    """an OracleShardEngine for its combine() alone: no camera is built"""
    e = OracleShardEngine.__new__(OracleShardEngine)
    e.bw, e.bh, e.balance = bw, bh, balance
    return e


def synthetic_runs(bw, bh):
    for k, (name, boxes) in enumerate(K.synthetic(bw, bh).items()):
        for fill in K.FILLS:
            yield name, boxes, fill, K.fill_parts(boxes, fill, k)


@pytest.mark.parametrize("bw,bh", K.SYNTH_BEVS)
def test_statement_equals_the_add_sat_chain(oracle, bw, bh):
    for name, boxes, fill, parts in synthetic_runs(bw, bh):
        for car_kind in K.CARS:
            car = K.make_car(bw, bh, car_kind)
            for balance in (False, True):
                want = chain_engine(bw, bh, balance).combine(parts, boxes, car)
                got = K.combine_statement(parts, boxes, bw, bh, car, balance)
                assert np.array_equal(got, want), "%d x %d %s, %s parts, %s car, balance %d" % (bw, bh, name, fill, car_kind, balance)


def shifted(boxes, bw, bh):
    """every box moved by one pixel in x (towards the side that has room)"""
    return [(x0 + 1, y0, x1 + 1, y1) if x1 < bw else (x0 - 1, y0, x1 - 1, y1) for x0, y0, x1, y1 in boxes if not (x0 == 0 and x1 == bw)]


def off_by_a_row(p):
    """the part read with its image stride one row short: image b starts a row early"""
    flat = np.concatenate([p.reshape(-1), np.zeros(p.shape[2] * 3, np.uint8)])
    row, img = p.shape[2] * 3, (p.shape[1] - 1) * p.shape[2] * 3
    return np.stack([flat[b * img:b * img + p.shape[1] * row].reshape(p.shape[1:]) for b in range(p.shape[0])])


@pytest.mark.parametrize("bw,bh", K.SYNTH_BEVS)
def test_statement_negative_controls(oracle, bw, bh):
    caught = dict(shift=[], stride=[], wrap=[])
    for name, boxes, fill, parts in synthetic_runs(bw, bh):
        want = chain_engine(bw, bh, False).combine(parts, boxes, None)
        moved = shifted(boxes, bw, bh)
        if len(moved) == len(boxes) and not np.array_equal(K.combine_statement(parts, moved, bw, bh), want):
            caught["shift"].append((name, fill))
        if not np.array_equal(K.combine_statement([off_by_a_row(p) for p in parts], boxes, bw, bh), want):
            caught["stride"].append((name, fill))
        if not np.array_equal((K.part_sums(parts, boxes, bw, bh) & 255).astype(np.uint8), want):
            caught["wrap"].append((name, fill))
    print({k: len(v) for k, v in caught.items()})
    assert all(caught.values()), caught
    # a shifted 1 x 1 box is seen; a wrapping add is seen exactly where parts overlap; every fill but all-255 sees the stride
    assert ("corners_1x1", "random") in caught["shift"] and ("stack8", "white") in caught["wrap"] and ("disjoint", "high") not in caught["wrap"]
    assert ("build4", "random") in caught["stride"] and ("build4", "white") not in caught["stride"]
