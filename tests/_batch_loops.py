"""What the batch-loop tests of the one-channel, 16-bit, nearest, packed 4:2:2 and moving kernels share (tests/test_batch_loops_gpu.py, its
worker tests/_batch_loops_worker.py and the host leg tests/test_batch_loops_host.py): the cases, their pools and yardsticks, and the runners
over tests/_harness.run_batches.  Imported as `tests._batch_loops`; the library is loaded inside the functions that need it.

k_units_gray, k_units_gray16, k_units_nn8 / k_units_nn16 and k_stitch_units_gray all run mono_unit_run (csrc/bevw_mono_unit.h), the one-channel form of plan_unit_run's frame loop (b_begin /
b_end, frame_of, issue(b + 2), land(ring ^ 1), two frames per step); k_units_yuv422 is a new instantiation of the shared one, and
k_stitch_moving has a loop and a chunk rule (moving_nb) of its own.  tests/test_batch_chunks_gpu.py says what such a loop gets wrong and how
the batch sizes of H.BATCHES were chosen; plan_args is shared, so the table H.PLAIN applies to every unit kernel here unchanged.

Every frame of a pool is distinct, full-range and uniform random -- the nearest cases too: on label frames a wrong frame's image could equal
the right one.  Yardsticks, all at tolerance 0: oracle.remap on the 2-D uint8 / uint16 array (linear remappers), tests/_nearest.want_nn
(nearest), tests/_gray_stitch.spec over the oracle (one-channel stitch), RefBevGenerator (4:2:2 stitch on the specification's BGR frames;
moving stitch with the rig of each frame set)."""
import numpy as np

from tests import _caller_maps as CM
from tests import _far_batches as FB
from tests import _gray_stitch as GS
from tests import _harness as H
from tests import _moving as MV
from tests import _nearest as N

POOL = 143                                  # distinct frames / frame sets; a batch of B is the first B of them
CFG = H.SMALL_CFG

# ---------------------------------------------------------------------------------------------------------------
# one-channel remappers: 320 x 256 -> 640 x 512, the geometry of the undistorter of tests/test_batch_chunks_gpu.py
# ---------------------------------------------------------------------------------------------------------------
REMAP_SIZE = (320, 256, 640, 512)           # sw, sh, dw, dh
# The fisheye map of small_rig()'s front camera at these sizes keeps every footprint inside the frame: 80 units, none without a contributor,
# no base tile for the per-tap kernels (tests/test_batch_loops_host.py asserts it, so that a change of the rig brings the choice up again).
# `swirl_wide` of tests/_caller_maps.py leaves the frame over its whole outer ring: units whose `ngroups == 0` loop runs AND base tiles on
# the frame border for k_stitch_plan_gray / k_stitch_plan_gray16 / k_tiles_nn8 / k_tiles_nn16.
REMAP_FAMILY = "swirl_wide"
REMAPPERS = (("linear", 8), ("linear", 16), ("nearest", 8), ("nearest", 16))   # (interpolation, depth)
DTYPE = {8: np.uint8, 16: np.uint16}


def remap_maps():
    return CM.family(REMAP_FAMILY, *REMAP_SIZE)


def front_maps(oracle):
    """The fisheye undistort maps of small_rig()'s front camera at REMAP_SIZE."""
    sw, sh, dw, dh = REMAP_SIZE
    K, D, _ = H.small_rig()["front"]
    return oracle.fisheye_init_undistort_rectify_map(K, D, oracle.camera_mat_dst(K, sw, sh, CFG["FOCAL_SCALE"], CFG["SIZE_SCALE"]), (dw, dh))


def remap_frames(depth, n=POOL):
    """n distinct frames [n, sh, sw] of uniform random texels over the full range of the depth."""
    sw, sh = REMAP_SIZE[:2]
    return np.random.default_rng([2100, depth]).integers(0, 1 << depth, (n, sh, sw), dtype=DTYPE[depth])


def remap_want(oracle, kind, frames, maps):
    """-> (images [n, dh, dw] of the frames' type, the pixels no frame reaches: 0 there)"""
    sw, sh = REMAP_SIZE[:2]
    if kind == "nearest":
        return N.want_nn(frames, *maps), ~N.inside_nn(maps[0], maps[1], sw, sh)
    return np.stack([oracle.remap(f, *maps) for f in frames]), H.outside_of(maps[0], sw, sh)


class OneChannelRemapper(H.Remapper):
    """H.Remapper with one channel at `depth` bits and the given interpolation."""

    def __init__(self, ffi, kind, depth):
        super().__init__(ffi, remap_maps(), REMAP_SIZE, channels=1)
        self.kind, self.depth = kind, depth

    def __enter__(self):
        super().__enter__()
        try:
            N.set_depth(self, self.depth)
            N.set_interpolation(self, self.kind == "nearest")
        except Exception:
            self.L.bevw_remapper_destroy(self.r)
            raise
        return self


def run_remapper(ffi, kind, depth, d_src, want, batches, nb_env=0):
    """One remapper over `batches` through bevw_remap_device on the device-resident pool d_src; every step on the units."""
    dw, dh = REMAP_SIZE[2:]
    what = "remap %s, depth %d" % (kind, depth)
    with OneChannelRemapper(ffi, kind, depth) as r:
        def sync():
            ffi.check(r.L.bevw_remapper_sync(r.r))
            assert r.last_path() == ffi.PATH_UNITS, "%s: path %d, not the units" % (what, r.last_path())

        launch = lambda B, d_out: ffi.check(r.L.bevw_remap_device(r.r, d_src.ptr, B, d_out.ptr))
        H.run_batches(ffi, launch, sync, dw * dh * depth // 8, False, dw, dh, dw, batches, (want[0], None, want[1]), what, nb_env=nb_env,
                      plane=DTYPE[depth])


# ---------------------------------------------------------------------------------------------------------------
# BevGenerator(channels=1)
# ---------------------------------------------------------------------------------------------------------------
def gray_pool(n=POOL, cfg=CFG, seed=2110):
    """(n distinct full-range frame sets [n, 4, FH, FW], a grey car sprite)"""
    rng = np.random.default_rng(seed)
    return GS.gray_frames(rng, cfg, n, dim=False), GS.gray_car(rng, cfg)


def gray_want(oracle, frames, car, blend, cfg=CFG):
    """-> (images [n, BH, BW], the pixels no camera covers: the car there)"""
    ref = oracle.RefBevGenerator(H.small_rig(), cfg, blend=blend)
    none = H.uncovered(ref)
    assert none.any()
    return GS.spec_batch(oracle, ref, frames, car), none


def run_gray_stitch(ffi, SB, d_in, d_car, car, want, blend, batches, cfg=CFG, nb_env=0, **kw):
    """One BevGenerator(channels=1) over `batches` through run_device on the device-resident pool; every step on the units."""
    what = "grey stitch, blend %d, %s" % (blend, kw)
    bev = H.generator(SB, H.small_rig(), cfg, channels=1, blend=blend, **kw)

    def sync():
        bev.sync()
        assert bev.last_path() == ffi.PATH_UNITS, "%s: path %d, not the units" % (what, bev.last_path())

    launch = lambda B, d_out: bev.run_device(d_in.ptr, B, d_car.ptr, d_out.ptr, out_bytes=d_out.nbytes)
    H.run_batches(ffi, launch, sync, bev.out_image_bytes, False, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], bev.out_pitch, batches,
                  (want[0], None, want[1]), what, nb_env=nb_env, plane=np.uint8, under=car)
    return bev


# ---------------------------------------------------------------------------------------------------------------
# YUYV / UYVY stitch: one pool of bytes, read in either order
# ---------------------------------------------------------------------------------------------------------------
def yuv422_pool(n=POOL, seed=2120):
    """(n distinct uniform random packed 4:2:2 frame sets, a car sprite); the same bytes serve as YUYV and as UYVY"""
    from tests import _yuv422_spec as S

    rng = np.random.default_rng(seed)
    return S.random_yuv422(rng, (n, 4), CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]), H.random_car(rng, CFG)


def yuv422_bgr(raw, order):
    from tests import _yuv422_spec as S

    return np.stack([S.yuv422_to_bgr(raw[b], order) for b in range(raw.shape[0])])


# ---------------------------------------------------------------------------------------------------------------
# k_stitch_moving: geometry T of tests/_far_batches.py, frame set b on rig b % 7
# ---------------------------------------------------------------------------------------------------------------
MOVING_CFG = FB.CFG_T
MOVING_TILES = 4 * 63                        # ceil(248 / 64) x ceil(250 / 4) tiles of 64 x 4 pixels
MOVING_BATCHES = (67, 131, 259, 33, 9)       # in this order on one handle: the nb = 4, 8, 16 blocks with a ragged last one, then shrinking
# batch -> (nb, blocks, frame sets of the last block) as moving_nb gives them on MOVING_TILES tiles (held against csrc/bevw_moving.h on the host)
MOVING = {67: (4, 17, 3), 131: (8, 17, 3), 259: (16, 17, 3), 33: (2, 17, 1), 9: (1, 9, 1)}
MOVING_POOL = max(MOVING_BATCHES)
MOVING_RIGS = (("pitch +0.5", "x", 0.5), ("pitch -2", "x", -2.0), ("yaw 1", "y", 1.0), ("roll 1", "z", 1.0), ("own H", "x", 0.0),
               ("pitch +1.5", "x", 1.5), ("roll -1.5", "z", -1.5))   # seven: coprime to every nb


def moving_rigs(oracle, cfg=MOVING_CFG):
    rig = FB.scaled_rig(cfg)
    return [(name, MV.with_h(rig, lambda n, K, Hm, ax=ax, deg=deg: MV.rotated(oracle, K, Hm, cfg, ax, deg))) for name, ax, deg in MOVING_RIGS]


def moving_pool(seed=2130):
    rng = np.random.default_rng(seed)
    cfg = MOVING_CFG
    frames = rng.integers(0, 256, (MOVING_POOL, 4, cfg["FRAME_HEIGHT"], cfg["FRAME_WIDTH"], 3), dtype=np.uint8)
    return frames, H.random_car(rng, cfg)


def moving_want(oracle, rigs, frames, car, blend):
    """-> (images [n, BH, BW, 3]: frame set b through RefBevGenerator(rig b % 7), None, the pixels no camera covers under the rig's own H)"""
    refs = [oracle.RefBevGenerator(r, MOVING_CFG, blend=blend) for _, r in rigs]
    none = np.all([H.uncovered(ref) for ref in refs], axis=0)   # covered by no camera under any of the seven rigs
    return np.stack([refs[b % len(refs)](*frames[b], car) for b in range(frames.shape[0])]), None, none


# ---------------------------------------------------------------------------------------------------------------
# the negative control: what a frame_of() clamp that is wrong by one leaves in the images
# ---------------------------------------------------------------------------------------------------------------
def wrong_clamp(images, nb):
    """images [B, ...] as a correct step leaves them -> as a step leaves them whose chunks run one frame past their end unclamped: the
    image of every chunk's first frame but the first chunk's holds the previous frame's (the last of the chunk before)."""
    out = images.copy()
    for b in range(nb, images.shape[0], nb):
        out[b] = images[b - 1]
    return out
