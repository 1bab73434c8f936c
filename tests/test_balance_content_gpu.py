"""The balance chain (balance=True) on the GPU with frame sets whose brightness and colour cast differ per set, camera and channel: the
pool of tests/_balance_content.py (33 sets: 26 graded ones with pairwise distinct delta tuples and gains from 0.59 to 1.84, and black,
white, three-black-one-white, dead-channel, near-dead-channel, dark and rounding-tie sets at fixed positions), whose preconditions
tests/test_balance_content_host.py asserts without a GPU: taking the deltas or gains of a neighbouring set, of the slice's first set or
of another camera changes the oracle's image of every graded set, so an index of the chain that is wrong by a set, a camera, a ring slot
or a clamped step fails here.

Tolerance 0 everywhere, against the CPU oracle on the frames (NV12 / YUYV / UYVY input: on the spec-converted frames; NV12 images: through
_nv12_out_spec).  The stitch cases reuse Inputs, Expected, run_batches, stitch_handle and check_image of tests/_harness.py
with this pool -- their 0x5A fill, their guard image and the reversed host-entry run -- with batches 33 (two slices of 16 and 17 frame
sets, chunks of 2) and 9 (one slice, chunks of 1) in that order on one handle.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest

from tests import _balance_content as BC
from tests import _nv12_out_spec as SO
from tests import _harness as H
from tests._harness import SB, ffi, run_child  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = BC.CFG
BATCHES = (33, 9)
OF = {"bgr": "bgr", "nv12": "nv12", "surfaces": "nv12", "yuyv": "yuyv", "uyvy": "uyvy"}   # input kind -> the form of the pool it reads


@pytest.fixture(scope="module")
def car():
    return BC.car()


@pytest.fixture(scope="module")
def inputs(ffi, car):
    i = H.Inputs(ffi, BC.forms("nv12")[0], BC.bgr_pool(), car, yuv422={o: BC.forms(o)[0] for o in ("yuyv", "uyvy")})
    yield i
    i.free()


@pytest.fixture(scope="module")
def expected(oracle, car):
    """form of the pool -> Expected: the oracle's images of the 33 sets per (blend, balance), computed on first use."""
    made = {}

    def get(form):
        form = "yuyv" if form == "uyvy" else form   # the same texels (tests/test_balance_content_host.py asserts it)
        if form not in made:
            made[form] = H.Expected(oracle, BC.forms(form)[1], car, CFG, BC.N)
        return made[form]

    return get


# ---------------------------------------------------------------------------------------------------------------
# a. the tile plan: every input kind x output format, blend off and on; the dense layout
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("inp", ["bgr", "nv12", "surfaces", "yuyv", "uyvy"])
def test_tile_plan_matches_oracle(ffi, SB, inputs, expected, inp, out, blend):
    bev = H.stitch_handle(ffi, SB, inputs, expected(OF[inp])(blend, True), inp, out, blend, True, batches=BATCHES)   # (asserts the unit schedule)
    assert bev.out_pitch == 256 and ffi.lib().bevw_input_format(bev._engine.h) == ffi.INPUT_FORMATS[OF[inp]]


@pytest.mark.parametrize("blend", [False, True])
def test_tile_plan_dense_layout(ffi, SB, inputs, expected, blend):
    bev = H.stitch_handle(ffi, SB, inputs, expected("bgr")(blend, True), "bgr", "bgr", blend, True, batches=BATCHES, output_pitch="dense")
    assert bev.out_pitch == CFG["BEV_WIDTH"]


# ---------------------------------------------------------------------------------------------------------------
# b. BEV width 250, dense: the plan's padded scratch, so a balance step of 33 is ONE slice; 250 x 251 images are no multiple of 4 pixels:
#    the byte-wise gain kernel, in place, with the sums of k_reduce_psums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bh", [250, 251])
def test_padded_scratch_one_slice_of_33(ffi, SB, oracle, inputs, bh):
    cfg = dict(CFG, BEV_WIDTH=250, BEV_HEIGHT=bh)
    car = H.random_car(np.random.default_rng(7250 + bh), cfg)
    want_bgr, _, none = H.Expected(oracle, BC.bgr_pool(), car, cfg, BC.N, nv12=False)(True, True)
    padded = H.Inputs(ffi, inputs.nv, inputs.bgr, car)
    padded.bufs["bgr"] = inputs.packed("bgr")
    try:
        bev = H.stitch_handle(ffi, SB, padded, (want_bgr, None, none), "bgr", "bgr", True, True, batches=(33,), cfg=cfg, one_slice=True,
                               output_pitch="dense")
        assert bev.out_pitch == 250 and (250 * bh) % 4 == (0 if bh == 250 else 2)
    finally:
        padded.car.free()


# ---------------------------------------------------------------------------------------------------------------
# c. the per-pixel schedule: the luminance round trip per tap, V sums and deltas of the whole batch in one pass
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("inp", ["bgr", "nv12"])
def test_per_pixel_schedule(ffi, SB, inputs, expected, inp, out, blend):
    bev = H.generator(SB, H.small_rig(), CFG, blend=blend, balance=True, schedule=ffi.SCHED_PER_PIXEL, input_format=inp, output_format=out)
    assert bev.plan_info()["schedule"] == ffi.SCHED_PER_PIXEL
    d_in, d_car = inputs.packed(inp), inputs.car.ptr
    launch = lambda B, d_out: bev.run_device(d_in.ptr, B, d_car, d_out.ptr, out_bytes=d_out.nbytes)
    H.run_batches(ffi, launch, bev.sync, bev.out_image_bytes, out == "nv12", CFG["BEV_WIDTH"], CFG["BEV_HEIGHT"], bev.out_pitch, (9,),
                   expected(inp)(blend, True), "per pixel, %s -> %s, blend %d" % (inp, out, blend))


@pytest.mark.parametrize("out", ["bgr", "nv12"])
def test_per_pixel_fallback_odd_frames(ffi, SB, oracle, out):
    """321 x 255 frames in the graded content (generated at that size: the pool's frames are narrower), batch 5: frames of 245565 bytes,
    no multiple of 4 or 12, so k_vsum takes single bytes and has tail texels, and the automatic schedule serves every tile per pixel."""
    cfg = dict(CFG, FRAME_WIDTH=321, FRAME_HEIGHT=255)
    frames = BC.graded(np.random.default_rng([BC.SEED, 321]), 5, 321, 255)
    car = H.random_car(np.random.default_rng([BC.SEED, 255]), cfg)
    bev = H.generator(SB, H.small_rig(), cfg, blend=True, balance=True, output_format=out)
    assert bev.plan_info()["tiles_staged"] == 0
    ref = oracle.RefBevGenerator(H.small_rig(), cfg, blend=True, balance=True)
    none = H.uncovered(ref)
    chain = BC.Chain(oracle, True, cfg)
    deltas = [chain.deltas(f) for f in frames]
    assert len(set(deltas)) == 5 and all(any(d) for d in deltas), deltas   # the content has teeth at this size too
    got = bev.batch(frames, car)
    for b in range(5):
        want = ref(*frames[b], car)
        H.check_image(got[b], want, none, "321 x 255 frames -> %s, set %d of 5" % (out, b), out, want_nv12=SO.bgr_to_nv12(want) if out == "nv12" else None)


# ---------------------------------------------------------------------------------------------------------------
# d. the balance switches, each set in a fresh child (the library reads them once per process)
# ---------------------------------------------------------------------------------------------------------------
SWITCHES = {"parts8_ring": {"BEVW_BAL_PARTS": "8", "BEVW_BAL_RING": "1"}, "parts5_ring": {"BEVW_BAL_PARTS": "5", "BEVW_BAL_RING": "1"},
            "parts7": {"BEVW_BAL_PARTS": "7", "BEVW_BAL_RING": "0"}, "per_tap_round_trip": {"BEVW_BAL_MODE": "0"},
            "gain_in_place": {"BEVW_GAIN_OOP": "0"}}
CHILD_TIMEOUT = 180   # seconds: a library load, two small handles and their four steps take a few seconds


@pytest.fixture(scope="module")
def case_dir(expected, car, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("balance_content"))
    want_bgr, _, none = expected("bgr")(True, True)
    want_nv12, want_nv12_out, _ = expected("nv12")(True, True)
    files = dict(nv=BC.forms("nv12")[0], bgr=BC.bgr_pool(), car=car, want_bgr=want_bgr, want_nv12=want_nv12, want_nv12_out=want_nv12_out, none=none)
    for name, a in files.items():
        np.save(os.path.join(d, name + ".npy"), a)
    return d


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_balance_switches(case_dir, switch):
    sw = SWITCHES[switch]
    args = ["%s=%s" % kv for kv in sorted(sw.items())]
    run_child("_balance_content_worker.py", [case_dir] + args, sw, ("BEVW_BAL_", "BEVW_GAIN_", "BEVW_PLAN_"), CHILD_TIMEOUT, "worker OK %s" % " ".join(args))


# ---------------------------------------------------------------------------------------------------------------
# e. camera shards in one process: V sums per shard, the host gather into [batch][4], partial stitches, pack, combine
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", [[(0, 1, 2, 3)], [(0, 1), (2, 3)], [(0,), (1,), (2,), (3,)]], ids=["1_shard", "2_shards", "4_shards"])
def test_camera_shards(ffi, SB, oracle, expected, car, part):
    from cameracalibration_amd import workloads as W
    from cameracalibration_amd.SurroundBirdEyeView import cameraShard as CS

    frames = np.ascontiguousarray(BC.bgr_pool()[:9])
    want = expected("bgr")(True, True)[0][:9]
    full = H.generator(SB, H.small_rig(), CFG, blend=True, balance=True, output_pitch="dense")   # (also leaves CFG in the shared arguments)
    CS._sb.BevGenerator.init_args(None)
    rig_list = [H.small_rig()[n] for n in W.CAMERA_NAMES]
    engines = [CS.HipShardEngine(rig_list, cams, True, True) for cams in part]
    try:
        vsums = np.zeros((9, 4), np.uint64)
        for e in engines:
            vsums[:, list(e.cams)] = e.vsums(np.ascontiguousarray(frames[:, list(e.cams)]))   # bevw_shard_vsums_device
        assert vsums.tolist() == [[oracle.sum_v(frames[b, k]) for k in range(4)] for b in range(9)]
        parts = [e.partial(np.ascontiguousarray(frames[:, list(e.cams)]), vsums) for e in engines]   # bevw_shard_run_device, bevw_shard_pack_device
        got = engines[-1].combine(parts, [e.box for e in engines], car)                              # bevw_combine_device
    finally:
        for e in engines:
            e.close()
    stitched = full.batch(frames, car)
    for b in range(9):
        what = "%d shards, set %d (%s)" % (len(part), b, BC.SPECIAL.get(b, "graded"))
        assert np.array_equal(got[b], want[b]), "%s: %d bytes differ from the oracle" % (what, np.count_nonzero(got[b] != want[b]))
        assert np.array_equal(got[b], stitched[b]), "%s: differs from the full stitch" % what


# ---------------------------------------------------------------------------------------------------------------
# f. the exported helpers through the C ABI, batch > 1, under both addWeighted variants
# ---------------------------------------------------------------------------------------------------------------
LUM_SETS = (2, 3, 5, 7, 8)   # graded, three black and one white, dead channel, tie, graded


def balance_images(w, h, seed):
    """Five images for bevw_color_balance: dead channel, near-dead channel, dark, a graded cast, exact ties.  The last one has channel values
    symmetric about the means 40 / 60 / 80 (39 | 41, 59 | 61, 78 | 82 in equal numbers; at an odd pixel count one pixel of 40, 60, 80): the
    gains are exactly 1.5, 1.0 and 0.75, and every gained B and R byte is a .5 tie (58.5 | 61.5)."""
    rng = np.random.default_rng([seed, w, h])
    dead = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    dead[..., 0] = 0
    near = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    near[..., 0] = 0
    near.reshape(-1, 3)[rng.choice(w * h, 5, replace=False), 0] = 1
    dark = rng.integers(0, 4, (h, w, 3), dtype=np.uint8)
    cast = ((rng.integers(0, 256, (h, w, 3)) * np.array([230, 90, 160])) >> 8).astype(np.uint8)
    n = w * h
    side = np.zeros(n, np.int64)
    side[:n // 2], side[n // 2:2 * (n // 2)] = -1, 1   # an odd pixel count leaves one 0
    tie = np.stack([40 + rng.permutation(side), 60 + rng.permutation(side), 80 + 2 * rng.permutation(side)], -1).astype(np.uint8).reshape(h, w, 3)
    return np.stack([dead, near, dark, cast, tie])


@pytest.mark.parametrize("addweighted", [1, 0])
def test_exported_helpers_batches(ffi, oracle, addweighted):
    L = ffi.lib()
    try:
        ffi.check(L.bevw_set_compat(ffi.COMPAT_ADDWEIGHTED, addweighted))
        oracle.set_variant(oracle.VARIANT_ADDWEIGHTED, addweighted)
        pool, chain = BC.bgr_pool(), BC.Chain(oracle, False)
        for w, h in ((320, 256), (53, 37)):
            frames = np.ascontiguousarray(pool[list(LUM_SETS), :, :h, :w])
            got = np.full_like(frames, H.FILL)
            ffi.check(L.bevw_luminance_balance(0, ffi.ptr(frames), 5, w, h, ffi.ptr(got)))
            deltas = [chain.deltas(f) for f in frames]
            assert len(set(deltas)) == 5, deltas
            for i in range(5):
                want = oracle.luminance_balance(list(frames[i]))
                for c in range(4):
                    assert np.array_equal(got[i, c], want[c]), "bevw_luminance_balance %d x %d, set %d of the batch (pool set %d, deltas %s), camera %d" % (
                        w, h, i, LUM_SETS[i], deltas[i], c)
        for w, h in ((64, 48), (77, 123)):
            imgs = balance_images(w, h, BC.SEED)
            got = np.full_like(imgs, H.FILL)
            ffi.check(L.bevw_color_balance(0, ffi.ptr(imgs), 5, w, h, ffi.ptr(got)))
            gains = [chain.gains(im) for im in imgs]
            assert np.isinf(gains[0][0]) and 255 < gains[1][0] < np.inf and gains[4].tolist() == [1.5, 1.0, 0.75], gains
            for i, name in enumerate(("dead channel", "near-dead channel", "dark", "graded cast", "exact ties")):
                want = oracle.color_balance(imgs[i])
                assert np.array_equal(got[i], want), "bevw_color_balance %d x %d, addWeighted variant %d, image %d (%s): %s" % (
                    w, h, addweighted, i, name, H.first_difference(got[i], want))
    finally:
        L.bevw_set_compat(ffi.COMPAT_ADDWEIGHTED, 1)
        oracle.set_variant(oracle.VARIANT_ADDWEIGHTED, 1)
