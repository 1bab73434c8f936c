"""The catalogue of the camera-shard tests (tests/test_shard_cases_host.py, tests/test_shard_cases_gpu.py): BEV geometries whose mask boxes
differ in kind from those of SMALL_CFG, camera partitions, frame content, rig families at the shard plan, and synthetic part lists for
bevw_combine_device; with it the NumPy statement of the combine and the census that keeps a case from passing emptily.

Every recorded value below (BOXES, SATURATED, the floors) comes from the ORACLE's masks and images (oracle/oracle.py through
tests/_shard_oracle.OracleShardEngine), none from the library under test; tests/test_shard_cases_host.py asserts that a run reproduces them.

A shard's part is the saturating sum of its cameras' masked images on the bounding box of their masks, x widened to multiples of 4 and
cut at the BEV; an empty mask gives the box (0, 0, 4, 1).  Boxes are (x0, y0, x1, y1)."""
import numpy as np

from tests import _rigs as R
from tests import _shard_common as SC
from tests._harness import SMALL_CFG, small_rig
from tests._shard_oracle import OracleShardEngine, mask_box

# (BEV_WIDTH, BEV_HEIGHT, CAR_WIDTH, CAR_HEIGHT), all on small_rig() with frames 320 x 256
GEOMETRIES = (
    (253, 255, 63, 101),   # bw % 4 == 1, `right` 97 wide: the byte paths of pack and combine
    (270, 270, 50, 88),    # bw % 4 == 2, `right` 110 wide
    (260, 250, 62, 250),   # car as tall as the BEV: direct `back` is empty (the fallback box), direct `front` is one row
    (260, 250, 260, 100),  # car as wide as the BEV: direct `right` is empty, direct `left` one column widened to 4
    (300, 96, 150, 40),    # wide
    (96, 300, 20, 200),    # tall
    (252, 180, 0, 0),      # no car, the masks meet in the centre: the one geometry whose blend parts saturate before the car
    (64, 48, 13, 21),      # small, odd car
)
ALL_MODES = ((253, 255, 63, 101), (260, 250, 62, 250))   # these run all four (blend, balance) pairs on the GPU
MODES = ((False, False), (True, True))
FOUR_MODES = ((False, False), (True, False), (False, True), (True, True))

# the five of tests/test_camera_shard.py (the host module asserts that they still are) and two more
PARTITIONS = ([(0, 1, 2, 3)], [(0, 1), (2, 3)], [(0,), (1,), (2,), (3,)], [(0, 2), (1, 3)], [(0,), (1, 2, 3)], [(0, 3), (1, 2)], [(0, 1, 2), (3,)])
SINGLES = PARTITIONS[2]
RIG_FAMILIES = ("sideways", "mirrored", "roll90", "magnify", "minify4", "pincushion", "offcentre", "same4", "anisotropic")
RIG_PARTITIONS = ([(0,), (1, 2, 3)], SINGLES)
RIG_BATCH = 2
assert set(R.BORDER) <= set(RIG_FAMILIES)

SYNTH_BEVS = ((248, 250), (250, 251), (249, 251))   # the dword kernel (where boxes and pointers allow it), and the byte kernel twice
SYNTH_BATCH = 3
FILLS = ("random", "high", "white")
CARS = ("none", "random", "white")


def geo_name(geo):
    return "%dx%d_car%dx%d" % geo


def geo_cfg(geo):
    return dict(SMALL_CFG, BEV_WIDTH=geo[0], BEV_HEIGHT=geo[1], CAR_WIDTH=geo[2], CAR_HEIGHT=geo[3])


def subject(kind, name):
    """-> (rig, cfg, frames [B, 4, FH, FW, 3], car) of a geometry (kind 'geo', name a GEOMETRIES entry) or a rig family (kind 'rig')"""
    if kind == "geo":
        cfg = geo_cfg(name)
        return small_rig(), cfg, SC.content(cfg), SC.car(cfg)
    rig, cfg = R.family(name)
    return rig, cfg, R.frames(cfg, RIG_BATCH), R.car(cfg)


class OracleShards:
    """The oracle's side of one (subject, blend, balance): shard engines by camera tuple (built once each), the V sums of all four cameras,
    and parts per partition.  The module arguments of surroundBEV are set to the subject's cfg while an engine is built."""

    def __init__(self, rig, cfg, frames, blend, balance):
        self.rig_list = [rig[n] for n in SC.W.CAMERA_NAMES]
        self.cfg, self.frames, self.blend, self.balance, self.engines, self._parts = cfg, frames, blend, balance, {}, {}
        self.all_vsums = None
        if balance:
            from oracle import oracle as O

            O.build()
            self.all_vsums = np.array([[O.sum_v(f) for f in fs] for fs in frames], np.uint64)

    def engine(self, cams):
        cams = tuple(cams)
        if cams not in self.engines:
            SC.apply_cfg(self.cfg)
            try:
                self.engines[cams] = OracleShardEngine(self.rig_list, cams, self.blend, self.balance)
            finally:
                SC.apply_cfg()
        return self.engines[cams]

    def part(self, cams):
        cams = tuple(cams)
        if cams not in self._parts:
            self._parts[cams] = self.engine(cams).partial(np.ascontiguousarray(self.frames[:, list(cams)]), self.all_vsums)
        return self._parts[cams]

    def combine(self, partition, car):
        e = self.engine(partition[-1])
        return e.combine([self.part(c) for c in partition], [self.engine(c).box for c in partition], car)


# ---------------------------------------------------------------------------------------------------------------
# the combine, stated in NumPy
# ---------------------------------------------------------------------------------------------------------------
def part_sums(parts, boxes, bw, bh):
    """integer sum over the parts covering each byte, [B, bh, bw, 3] int32 -- before any saturation"""
    acc = np.zeros((parts[0].shape[0], bh, bw, 3), np.int32)
    for p, (x0, y0, x1, y1) in zip(parts, boxes):
        assert p.shape[1:] == (y1 - y0, x1 - x0, 3), (p.shape, (x0, y0, x1, y1))
        acc[:, y0:y1, x0:x1] += p
    return acc


def combine_statement(parts, boxes, bw, bh, car=None, balance=False):
    """min(255, sum over the covering parts (+ car)); with balance min(255, sum), then O.color_balance per image, then the car"""
    acc = part_sums(parts, boxes, bw, bh)
    if not balance:
        return np.minimum(255, acc + (0 if car is None else car.astype(np.int32))).astype(np.uint8)
    from oracle import oracle as O

    out = np.stack([O.color_balance(img) for img in np.minimum(255, acc).astype(np.uint8)])
    return out if car is None else np.minimum(255, out.astype(np.int32) + car).astype(np.uint8)


def depth(boxes, bw, bh):
    """how many boxes cover each pixel, [bh, bw]"""
    d = np.zeros((bh, bw), np.int32)
    for x0, y0, x1, y1 in boxes:
        d[y0:y1, x0:x1] += 1
    return d


# ---------------------------------------------------------------------------------------------------------------
# synthetic part lists for bevw_combine_device
# ---------------------------------------------------------------------------------------------------------------
def build_boxes(bw, bh):
    """the boxes of the four single-camera shards at (bw, bh) with SMALL_CFG's car, blend masks (the oracle's)"""
    from oracle import oracle as O

    O.build()
    geo = (bw, bh, SMALL_CFG["CAR_WIDTH"], SMALL_CFG["CAR_HEIGHT"])
    return [mask_box([O.blend_mask_for(n, *geo)], bw, bh) for n in SC.W.CAMERA_NAMES]


def synthetic(bw, bh):
    """{name: boxes}: 1..8 boxes inside the BEV"""
    a = (bw - 8) & ~3   # an x aligned to 4 near the right edge
    return {
        "whole": [(0, 0, bw, bh)],
        "corners_1x1": [(0, 0, 1, 1), (bw - 1, 0, bw, 1), (0, bh - 1, 1, bh), (bw - 1, bh - 1, bw, bh)],
        "one_4x1": [(8, 5, 12, 6)],
        "rows_top_bottom": [(0, 0, bw, 1), (0, bh - 1, bw, bh)],
        "right_column": [(bw - 1, 0, bw, bh)],
        "x0_unaligned": [(1, 3, 41, 40), (2, 10, 50, 60), (3, 20, 23, 25), (bw - 7, bh - 9, bw - 3, bh)],     # widths are multiples of 4
        "width_unaligned": [(0, 0, 5, 7), (4, 2, 10, 9), (8, 4, 15, 30), (a, bh - 3, bw - 1, bh)],            # x0 is a multiple of 4
        "stack8": [(16, 16, 80, 48)] * 8,                                                                        # aligned: dwords where bw allows
        "stack8_ragged": [(16 - k, 16 + k, 60 + 3 * k, 40 + 2 * k) for k in range(8)],                         # all cover (16..60, 23..40)
        "overlap_aligned": [(0, 0, 128, 100), (64, 50, a, 200), (32, 75, 96, bh), (64, 90, 68, 91)],          # different y0 per part
        "disjoint": [(0, 0, 8, 4), (a - 8, bh - 6, a, bh - 2), (100, 100, 104, 101)],
        "build4": build_boxes(bw, bh),
    }


def fill_parts(boxes, fill, seed):
    """parts [SYNTH_BATCH, y1-y0, x1-x0, 3] per box: random bytes, bytes >= 128 (almost every overlap saturates), or all 255"""
    rng = np.random.default_rng(seed)
    lo = dict(random=0, high=128, white=255)[fill]
    return [rng.integers(lo, 256, (SYNTH_BATCH, y1 - y0, x1 - x0, 3), dtype=np.uint8) for x0, y0, x1, y1 in boxes]


def make_car(bw, bh, kind):
    """a car image over the WHOLE BEV (the combine takes any image): None, random bytes or all 255"""
    if kind == "none":
        return None
    return np.full((bh, bw, 3), 255, np.uint8) if kind == "white" else np.random.default_rng(11).integers(0, 256, (bh, bw, 3), dtype=np.uint8)


def synthetic_classes(bw, bh):
    """{class: [case names]} of the classes the synthetic catalogue has to hit at (bw, bh); 'saturated' with the `high` fill"""
    hit = dict(x0_unaligned=[], width_unaligned=[], more_than_4_parts=[], depth_3=[], saturated=[], dword_eligible=[])
    for k, (name, boxes) in enumerate(synthetic(bw, bh).items()):
        if any(b[0] % 4 for b in boxes):
            hit["x0_unaligned"].append(name)
        if any((b[2] - b[0]) % 4 for b in boxes):
            hit["width_unaligned"].append(name)
        if len(boxes) > 4:
            hit["more_than_4_parts"].append(name)
        d = depth(boxes, bw, bh)
        if d.max() >= 3:
            hit["depth_3"].append(name)
        sums = part_sums(fill_parts(boxes, "high", k), boxes, bw, bh)
        if (sums > 255).sum() * 2 > 3 * SYNTH_BATCH * (d > 0).sum():
            hit["saturated"].append(name)
        if bw % 4 == 0 and not any(b[0] % 4 or (b[2] - b[0]) % 4 for b in boxes):
            hit["dword_eligible"].append(name)
    return hit


# ---------------------------------------------------------------------------------------------------------------
# recorded on the oracle (tests/test_shard_cases_host.py asserts that a run reproduces them)
# ---------------------------------------------------------------------------------------------------------------
# boxes of the single-camera shards (front, back, left, right) per geometry, {blend: boxes}
BOXES = {
    (253, 255, 63, 101): {False: [(0, 0, 253, 78), (0, 178, 253, 255), (0, 0, 96, 255), (156, 0, 253, 255)],
                           True: [(0, 0, 253, 78), (0, 178, 253, 255), (0, 0, 96, 255), (156, 0, 253, 255)]},
    (270, 270, 50, 88): {False: [(0, 0, 270, 92), (0, 179, 270, 270), (0, 0, 112, 270), (160, 0, 270, 270)],
                           True: [(0, 0, 270, 92), (0, 179, 270, 270), (0, 0, 112, 270), (160, 0, 270, 270)]},
    (260, 250, 62, 250): {False: [(0, 0, 260, 1), (0, 0, 4, 1), (0, 0, 100, 250), (160, 0, 260, 250)],
                           True: [(0, 0, 260, 46), (0, 205, 260, 250), (0, 0, 100, 250), (160, 0, 260, 250)]},
    (260, 250, 260, 100): {False: [(0, 0, 260, 76), (0, 175, 260, 250), (0, 0, 4, 250), (0, 0, 4, 1)],
                           True: [(0, 0, 260, 76), (0, 175, 260, 250), (0, 0, 48, 250), (212, 0, 260, 250)]},
    (300, 96, 150, 40): {False: [(0, 0, 300, 29), (0, 68, 300, 96), (0, 0, 76, 96), (224, 0, 300, 96)],
                           True: [(0, 0, 300, 29), (0, 68, 300, 96), (0, 0, 76, 96), (224, 0, 300, 96)]},
    (96, 300, 20, 200): {False: [(0, 0, 96, 51), (0, 250, 96, 300), (0, 0, 40, 300), (56, 0, 96, 300)],
                           True: [(0, 0, 96, 58), (0, 243, 96, 300), (0, 0, 40, 300), (56, 0, 96, 300)]},
    (252, 180, 0, 0): {False: [(0, 0, 252, 91), (0, 90, 252, 180), (0, 0, 128, 180), (124, 0, 252, 180)],
                           True: [(0, 0, 252, 91), (0, 90, 252, 180), (0, 0, 128, 180), (124, 0, 252, 180)]},
    (64, 48, 13, 21): {False: [(0, 0, 64, 14), (0, 34, 64, 48), (0, 0, 28, 48), (36, 0, 64, 48)],
                           True: [(0, 0, 64, 14), (0, 34, 64, 48), (0, 0, 28, 48), (36, 0, 64, 48)]},
}
# bytes of the three frame sets of SC.content() (random, white, black) whose integer sum over the four single-camera parts exceeds 255,
# before the car, per geometry, {(blend, balance): counts}
SATURATED = {
    (253, 255, 63, 101): {(False, False): (278, 1407, 0), (True, True): (0, 0, 0)},
    (270, 270, 50, 88): {(False, False): (291, 1644, 0), (True, True): (0, 0, 0)},
    (260, 250, 62, 250): {(False, False): (204, 597, 0), (True, True): (0, 0, 0)},
    (260, 250, 260, 100): {(False, False): (67, 453, 0), (True, True): (0, 0, 0)},
    (300, 96, 150, 40): {(False, False): (218, 897, 0), (True, True): (0, 0, 0)},
    (96, 300, 20, 200): {(False, False): (195, 822, 0), (True, True): (0, 0, 0)},
    (252, 180, 0, 0): {(False, False): (432, 1740, 0), (True, True): (0, 6, 0)},
    (64, 48, 13, 21): {(False, False): (116, 315, 0), (True, True): (0, 0, 0)},
}
