"""Caller buffers at hostile DISTANCES and COUNTS: batches whose input or output runs past 2^31 and 2^32 bytes, and batches whose frames
exceed the 65535 blocks a grid holds in y or z.  The cases, their geometry and the index arithmetic shared by the worker
(tests/_far_batches_worker.py), its driver (tests/test_far_batches_gpu.py) and the host leg (tests/test_far_batches_host.py).

Every kernel forms base + (size_t)b * set_bytes by hand and every buffer descriptor takes a 32-bit size; one missing cast is invisible
below 4 GiB.  for_each_chunk (csrc/bevw_host.h) cuts what rides in grid.y / grid.z at 65535, and for k_vsum (frames, four per set) the first
cut falls at frame 65535 = set 16383, camera 3: inside a frame set.

Two geometries, both with dense images and the repo rig scaled as tests/_harness.random_rig_case scales it:
  F (far input)   SMALL_CFG: 983,040 bytes per BGR frame set.  The batch is derived from the INPUT: two sets past 2^32 bytes.
  T (far output, long batch)   frames 64 x 48 -> BEV 248 x 250: 36,864 bytes per set, 186,000 per image.  The batch is derived from the
                  OUTPUT: two images past 2^32 bytes -- 23,094 sets = 92,376 frames for BGR images, more than one grid of frames.
Nothing here provokes a fault: every pointer and every size handed to the library is valid.

Content: a pool of POOL = 7 distinct graded frame sets (brightness differs per camera and set), repeated over the batch; image b must be the
oracle's image of set b % 7.  7 is coprime to the 8- and 16-frame chunk sizes, so an image computed from a wrong base -- a neighbouring
set, a chunk off -- never lands on an equal one; a base that lost 2^32 bytes is no whole number of sets or images away (the host leg asserts
that no unit size here divides a boundary) and reads or writes across two of them."""
import collections

import numpy as np

from tests._harness import SMALL_CFG

POOL = 7
SEED = 1660
BOUNDARIES = (1 << 31, 1 << 32)
GRID_MAX = 65535
CFG_T = dict(FRAME_WIDTH=64, FRAME_HEIGHT=48, BEV_WIDTH=248, BEV_HEIGHT=250, CAR_WIDTH=62, CAR_HEIGHT=100, FOCAL_SCALE=1.0, SIZE_SCALE=2.0)
GEOMETRIES = {"F": (SMALL_CFG, "in"), "T": (CFG_T, "out")}     # cfg, the side whose bytes the batch is derived from
MODES = {"direct": (False, False), "balance": (True, True)}    # (blend, balance); 'balance' is blend + balance
VSUM_CUT = (16382, 16383, 16384, 16385)                        # the sets around frame 65535 = set 16383, camera 3
REMAP_SIZE = (64, 48, 248, 250)                                # sw, sh, dw, dh of the far remapper
REMAP_FAMILY = "swirl"                                         # of tests/_caller_maps.py: smooth inside, leaves the frame at the corners
COUNT_SIZE, COUNT_BATCH, COUNT_FAMILY = (8, 8, 8, 8), 65540, "scatter"   # remap_launch's cut: one grid of 65535 images and five more

# One-channel cases (tests/test_batch_loops_gpu.py covers their batch loops below 4 GiB): 62,000 bytes per image of the grey stitch on T,
# 124,000 per 16-bit image of the far remapper; depth / nearest describe a one-channel remapper.
# The moving stitch (bevw_run_homographies_device) runs 65,540 frame sets, five more than one grid: the cut of its launcher, whose second
# span starts at `minv + b0 * 36`.  MOVING_CFG is the smallest rung of a ladder of geometries tried on an MI355X (16 x 12 -> 32 x 32 and
# 64 x 64, 32 x 24 -> 64 x 64 and 124 x 126, 64 x 48 -> 124 x 126, each with a car and the rig scaled to it): every rung builds and its moving
# step equals the oracle, so the smallest one serves -- 2,304 bytes per frame set, 3,072 per dense image, 352 MB on the device in all.
MOVING_CFG = dict(FRAME_WIDTH=16, FRAME_HEIGHT=12, BEV_WIDTH=32, BEV_HEIGHT=32, CAR_WIDTH=8, CAR_HEIGHT=12, FOCAL_SCALE=1.0, SIZE_SCALE=2.0)
MOVING_BATCH = 65540
MOVING_RIGS = 7                                                # frame set b on rig b % 7 of tests/_batch_loops.moving_rigs

Case = collections.namedtuple("Case", "name kind geometry inp out schedule mode env depth nearest", defaults=(8, False))


def cases():
    c = []
    for mode in MODES:
        c.append(Case("F bgr->bgr plan %s" % mode, "stitch", "F", "bgr", "bgr", "plan", mode, {}))
    c.append(Case("F nv12->bgr plan direct", "stitch", "F", "nv12", "bgr", "plan", "direct", {}))
    for schedule in ("plan", "per_pixel"):
        for mode in MODES:
            c.append(Case("T bgr->bgr %s %s" % (schedule, mode), "stitch", "T", "bgr", "bgr", schedule, mode, {}))
    c.append(Case("T bgr->nv12 plan direct", "stitch", "T", "bgr", "nv12", "plan", "direct", {}))
    c.append(Case("remap far output", "remap", None, "bgr", "bgr", None, None, {}))
    c.append(Case("remap 65540 images", "remap_count", None, "bgr", "bgr", None, None, {"BEVW_REMAP_PLAN": "0"}))
    for schedule in ("plan", "per_pixel"):
        c.append(Case("T gray->gray %s" % schedule, "stitch_gray", "T", "gray", "gray", schedule, "direct", {}))
    c.append(Case("remap gray16 far output", "plane", None, "gray", "gray", None, None, {}, 16, False))
    c.append(Case("remap nn16 far output", "plane", None, "gray", "gray", None, None, {}, 16, True))
    c.append(Case("remap gray16 65540 images", "plane_count", None, "gray", "gray", None, None, {"BEVW_REMAP_PLAN": "0"}, 16, False))
    c.append(Case("remap nn8 65540 images", "plane_count", None, "gray", "gray", None, None, {"BEVW_REMAP_PLAN": "0"}, 8, True))
    c.append(Case("moving 65540 sets", "moving", None, "bgr", "bgr", None, "direct", {}))
    return c


def case(name):
    return {c.name: c for c in cases()}[name]


def scaled_rig(cfg):
    """The repo rig scaled to cfg's frame, undistorted grid and BEV, as tests/_harness.random_rig_case scales it."""
    from cameracalibration_amd import workloads as W

    fw, fh, bw, bh, ss = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], cfg["SIZE_SCALE"]
    A = np.diag([fw / 1280.0, fh / 1024.0, 1.0])
    U = np.diag([fw * ss / 2560.0, fh * ss / 2048.0, 1.0])
    Bm = np.diag([bw / 1000.0, bh / 1000.0, 1.0])
    return {n: (A @ K, D.copy(), Bm @ H @ np.linalg.inv(U)) for n, (K, D, H) in W.repo_rig().items()}


# ---------------------------------------------------------------------------------------------------------------
# index arithmetic, on plain integers
# ---------------------------------------------------------------------------------------------------------------
def straddler(unit_bytes, boundary):
    """The index of the one unit (frame set, image) of a dense array of them that starts below `boundary` and ends above it; None when a
    unit ends exactly on it."""
    return boundary // unit_bytes if boundary % unit_bytes else None


def far_batch(unit_bytes):
    """Units so that the array reaches two whole units past the unit that straddles 2^32."""
    return BOUNDARIES[-1] // unit_bytes + 3


def checked(batch, in_unit, out_unit, stride, extra=()):
    """{image index: why it is checked in full}: images 0 and 1, each straddler of the input and of the output offsets with its two
    neighbours, `extra`, the last two -- and every stride-th image of the rest."""
    why = {}

    def add(b, text):
        if 0 <= b < batch:
            why[b] = why[b] + "; " + text if b in why else text

    for b in range(0, batch, stride):
        add(b, "stride %d" % stride)
    add(0, "the first"), add(1, "the second")
    for side, unit in (("input", in_unit), ("output", out_unit)):
        for boundary in BOUNDARIES:
            s = straddler(unit, boundary)
            if s is not None:
                for d in (-1, 0, 1):
                    add(s + d, "%s2^%d of the %s bytes" % ({-1: "the last one below ", 0: "straddles ", 1: "the first one past "}[d],
                                                          boundary.bit_length() - 1, side))
    for b in extra:
        add(b, "around frame %d, the cut of a grid of frames" % GRID_MAX)
    add(batch - 2, "the last but one"), add(batch - 1, "the last")
    return why


def where(batch, b, why):
    """The position a failure names, in the manner of tests/_harness.where."""
    return "batch %d, image %d = pool set %d (%s)" % (batch, b, b % POOL, why)


def stride_for(batch):
    """A stride coprime to 7 and 16 that leaves about 2000 sampled images: one child stays within a few seconds of transfers."""
    s = max(3, batch // 2000) | 1
    while s % 7 == 0:
        s += 2
    return s


# ---------------------------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------------------------
def pool(cfg, inp):
    """(POOL frame sets in format `inp` as the engine takes them, the BGR sets the input specification makes of them, a car sprite)."""
    from tests import _balance_content as BC
    from tests import _nv12_spec as S
    from tests._harness import random_car

    rng = np.random.default_rng([SEED, cfg["FRAME_WIDTH"]])
    bgr = BC.graded(rng, POOL, cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"])
    car = random_car(rng, cfg)
    if inp == "bgr":
        return bgr, bgr, car
    assert inp == "nv12", inp
    native = np.stack([S.bgr_to_nv12(s) for s in bgr])
    return native, np.stack([S.nv12_to_bgr(s) for s in native]), car


def remap_pool(size):
    return np.random.default_rng([SEED, size[0], size[1]]).integers(0, 256, (POOL, size[1], size[0], 3), dtype=np.uint8)


def plane_pool(size, depth):
    """POOL distinct one-channel frames of uniform random texels over the full range of the depth."""
    return np.random.default_rng([SEED, size[0], size[1], depth]).integers(0, 1 << depth, (POOL, size[1], size[0]), dtype=np.uint8 if depth == 8 else np.uint16)


def gray_pool(cfg):
    """(POOL grey frame sets [POOL, 4, FH, FW]: channel 0 of the graded BGR pool, the grey car sprite)"""
    bgr, _, car = pool(cfg, "bgr")
    return np.ascontiguousarray(bgr[..., 0]), np.ascontiguousarray(car[..., 0])
