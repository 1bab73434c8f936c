"""The camera-per-GPU path on the catalogue of tests/_shard_cases.py, in one process through HipShardEngine / _ffi, tolerance 0 everywhere.

bevw_set_camera_shard + bevw_build (the mask bounding-box scan, a tile plan compiled for 1, 2 or 3 cameras), bevw_shard_vsums_device,
bevw_shard_run_device (k_lum_delta, k_delta_select, the unit schedule on a mostly empty BEV; k_shard_pp where a shard's own masks put
more than two cameras on a pixel and no tile plan exists), bevw_shard_pack_device (k_pack_box) and
bevw_combine_device (k_combine<4>, k_combine<1>, the white balance behind it) against the oracle:
  * geometries   per geometry, (blend, balance) pair and partition: the boxes, the V sums, every PACKED PART (not only the sum), and the
                 combine against oracle.RefBevGenerator and against the full BevGenerator of that geometry.  A geometry the full generator
                 builds also builds as shards, an owned camera with an empty mask included;
  * rig families the same four assertions on rigs unlike the sample rig, whose tables the 1- and 3-camera plans never met;
  * combine      bevw_combine_device on synthetic part lists (1 x 1 boxes, unaligned x0 and widths, 8 parts on one region, overlap that
                 saturates almost everywhere ...) on a direct, a blend and a balance handle, against the NumPy statement
                 (_shard_cases.combine_statement; tests/test_shard_cases_host.py pins it to the oracle's add chain).  The output is filled
                 with a sentinel and followed by a guard image; a part at ptr + 1, the car at ptr + 2, the output at ptr + 1 give the same bytes;
  * pack         bevw_shard_pack_device on random bytes instead of a stitch, at every box of a geometry, with d_full + 1 and d_packed + 1;
  * refusals     return -1, write nothing and leave the handle usable.
Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import _harness as H
from tests import _shard_cases as K
from tests import _shard_common as SC
from tests._harness import SB, ffi  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = H.FILL
GEO_MODES = [(g, m) for g in K.GEOMETRIES for m in (K.FOUR_MODES if g in K.ALL_MODES else K.MODES)]


def geo_mode_id(v):
    return K.geo_name(v) if len(v) == 4 else "blend%d_balance%d" % v


class shard_args:
    """the module arguments of surroundBEV set to cfg while shard handles are built (HipShardEngine snapshots them), SMALL_CFG after"""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        from cameracalibration_amd.SurroundBirdEyeView import cameraShard as CS

        SC.apply_cfg(self.cfg)
        CS._sb.BevGenerator.init_args(None)
        return CS

    def __exit__(self, *exc):
        from cameracalibration_amd.SurroundBirdEyeView import cameraShard as CS

        SC.apply_cfg()
        CS._sb.BevGenerator.init_args(None)
        return False


def hip_engine(cfg, rig_list, cams, blend, balance):
    with shard_args(cfg) as CS:
        return CS.HipShardEngine(rig_list, cams, blend, balance)


def check_subject(SB, oracle, kind, name, blend, balance, partitions):
    from cameracalibration_amd import _ffi

    rig, cfg, frames, car = K.subject(kind, name)
    bw, bh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    what = "%s %s blend %d balance %d" % (kind, name, blend, balance)
    orc = K.OracleShards(rig, cfg, frames, blend, balance)
    ref = oracle.RefBevGenerator(rig, cfg, blend=blend, balance=balance)
    want = np.stack([ref(*fs, car=car) for fs in frames])
    try:
        full = H.generator(SB, rig, cfg, blend=blend, balance=balance).batch(frames, car)
    finally:
        SC.apply_cfg()
    H.assert_equal(full, want, what + ": the full BevGenerator")
    engines, parts, per_pixel = {}, {}, False
    try:
        for part in partitions:
            for cams in part:
                if cams not in engines:
                    engines[cams] = hip_engine(cfg, orc.rig_list, cams, blend, balance)   # builds, an empty owned mask included
                assert engines[cams].box == orc.engine(cams).box, "%s, cameras %s: box" % (what, cams)
                # the tile plan holds two contributors per pixel: a shard whose masks never put more on one runs it, and nothing else
                most = int(np.sum([orc.engine((c,)).masks[c] != 0 for c in cams], axis=0).max())
                sched = engines[cams].schedule()
                assert sched == _ffi.SCHED_TILE_PLAN or (most > 2 and sched == _ffi.SCHED_PER_PIXEL), "%s, cameras %s: schedule %d with %d masks on a pixel" % (
                    what, cams, sched, most)
                per_pixel |= sched == _ffi.SCHED_PER_PIXEL
            all_vsums = None
            if balance:
                all_vsums = np.zeros((len(frames), 4), np.uint64)
                for cams in part:
                    all_vsums[:, list(cams)] = engines[cams].vsums(np.ascontiguousarray(frames[:, list(cams)]))
                assert np.array_equal(all_vsums, orc.all_vsums), "%s, partition %s: V sums" % (what, part)
            for cams in part:
                if cams not in parts:
                    parts[cams] = engines[cams].partial(np.ascontiguousarray(frames[:, list(cams)]), all_vsums)
                H.assert_equal(parts[cams], orc.part(cams), "%s, cameras %s, box %s: the packed part" % (what, cams, engines[cams].box))
            boxes = [engines[cams].box for cams in part]
            for e in (engines[part[-1]], engines[part[0]]):   # the stitch role rotates: any rank's handle combines
                got = e.combine([parts[cams] for cams in part], boxes, car)
                H.assert_equal(got, want, "%s, partition %s combined on the handle of %s" % (what, part, e.cams))
            H.assert_equal(got, full, "%s, partition %s against the full BevGenerator" % (what, part))
        got = engines[part[-1]].combine([parts[cams] for cams in part], boxes, None)
        H.assert_equal(got, np.stack([ref(*fs) for fs in frames]), "%s, partition %s, no car" % (what, part))
    finally:
        for e in engines.values():
            e.close()
    assert got.shape == (len(frames), bh, bw, 3)
    return per_pixel


@pytest.mark.parametrize("geo,mode", GEO_MODES, ids=geo_mode_id)
def test_geometries(SB, oracle, geo, mode):
    per_pixel = check_subject(SB, oracle, "geo", geo, mode[0], mode[1], K.PARTITIONS)
    # without a car three or four masks meet in the centre: the shards of 3 and 4 cameras have no tile plan there (k_shard_pp)
    assert per_pixel == (geo == (252, 180, 0, 0))


@pytest.mark.parametrize("mode", K.MODES, ids=geo_mode_id)
@pytest.mark.parametrize("name", K.RIG_FAMILIES)
def test_rig_families(SB, oracle, name, mode):
    check_subject(SB, oracle, "rig", name, mode[0], mode[1], K.RIG_PARTITIONS)


# ---------------------------------------------------------------------------------------------------------------
# bevw_combine_device on the synthetic part lists
# ---------------------------------------------------------------------------------------------------------------
SLACK = 8   # bytes behind a buffer's payload, so that a copy may start at ptr + 1 or ptr + 2


class Pool:
    """device buffers of one test, freed together"""

    def __init__(self, ffi):
        self.ffi, self.bufs = ffi, []

    def new(self, nbytes):
        self.bufs.append(self.ffi.DeviceBuffer(nbytes + SLACK))
        return self.bufs[-1]

    def put(self, arr, offset=0):
        return self.new(arr.nbytes).upload(arr, offset).ptr + offset

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def combine_call(ffi, h, ptrs, boxes, batch, d_car, d_out):
    n = len(ptrs)
    arr = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in ptrs])
    bx = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1))
    return ffi.lib().bevw_combine_device(h, arr, ffi.ptr(bx), n, batch, d_car, d_out)


def run_into_sentinel(ffi, h, d_out, offset, nbytes, call, what):
    """d_out (nbytes payload + one guard image + SLACK) filled with the sentinel; call(ptr) writes nbytes at ptr = d_out + offset; -> the
    payload, after the bytes before it and the guard behind it were found untouched"""
    d_out.fill(FILL)
    ffi.check(call(d_out.ptr + offset))
    ffi.check(ffi.lib().bevw_sync(h))
    raw = d_out.download((d_out.nbytes,))
    assert (raw[:offset] == FILL).all(), what + ": bytes in front of the output were written"
    behind = raw[offset + nbytes:]
    assert (behind == FILL).all(), "%s: %d bytes of the guard behind the output were written (first at +%d)" % (
        what, int((behind != FILL).sum()), int(np.argmax(behind != FILL)))
    return raw[offset:offset + nbytes]


def synth_handles(SB, bw, bh):
    """{kind: (object that owns the handle, handle, balance)}: a direct 1-camera shard, a blend handle of all four cameras that is no
    shard, a blend + balance shard of all four"""
    cfg = dict(H.SMALL_CFG, BEV_WIDTH=bw, BEV_HEIGHT=bh)
    rig_list = [H.small_rig()[n] for n in SC.W.CAMERA_NAMES]
    direct = hip_engine(cfg, rig_list, (0,), False, False)
    balance = hip_engine(cfg, rig_list, (0, 1, 2, 3), True, True)
    try:
        blend = H.generator(SB, H.small_rig(), cfg, blend=True)
    finally:
        SC.apply_cfg()
    return dict(direct=(direct, direct.h, False), blend=(blend, blend._engine.h, False), balance=(balance, balance.h, True))


@pytest.mark.parametrize("kind", ["direct", "blend", "balance"])
@pytest.mark.parametrize("bw,bh", K.SYNTH_BEVS)
def test_combine_on_synthetic_parts(ffi, SB, oracle, bw, bh, kind):
    B, img = K.SYNTH_BATCH, bw * bh * 3
    handles = synth_handles(SB, bw, bh)
    owner, h, balance = handles[kind]
    pool, ran = Pool(ffi), 0
    try:
        d_out = pool.new((B + 1) * img)
        cars = {c: K.make_car(bw, bh, c) for c in K.CARS}
        d_cars = {c: (None, None) if car is None else (pool.put(car), pool.put(car, 2)) for c, car in cars.items()}
        for k, (name, boxes) in enumerate(K.synthetic(bw, bh).items()):
            for fill in K.FILLS:
                parts = K.fill_parts(boxes, fill, k)
                case = Pool(ffi)
                try:
                    ptrs = [case.put(p) for p in parts]
                    moved = [case.put(parts[0], 1)] + ptrs[1:]
                    for c in K.CARS:
                        want = K.combine_statement(parts, boxes, bw, bh, cars[c], balance)
                        variants = [("aligned", ptrs, d_cars[c][0], 0), ("part 0 at ptr + 1", moved, d_cars[c][0], 0), ("output at ptr + 1", ptrs, d_cars[c][0], 1)]
                        if cars[c] is not None:
                            variants.append(("car at ptr + 2", ptrs, d_cars[c][1], 0))
                        for vname, pp, d_car, off in variants:
                            what = "%d x %d %s handle, %s, %s parts, %s car, %s" % (bw, bh, kind, name, fill, c, vname)
                            got = run_into_sentinel(ffi, h, d_out, off, B * img, lambda p: combine_call(ffi, h, pp, boxes, B, d_car, p), what)
                            H.assert_equal(got.reshape(B, bh, bw, 3), want, what)
                            ran += 1
                finally:
                    case.free()
    finally:
        pool.free()
        for o, _, _ in handles.values():
            (o.close if hasattr(o, "close") else o._engine.close)()
    assert ran == 12 * 3 * (3 + 4 + 4)


# ---------------------------------------------------------------------------------------------------------------
# bevw_shard_pack_device on arbitrary content
# ---------------------------------------------------------------------------------------------------------------
PACK_CAMS = tuple(sorted({cams for part in K.PARTITIONS for cams in part}))


@pytest.mark.parametrize("geo", K.GEOMETRIES, ids=K.geo_name)
def test_pack_on_arbitrary_content(ffi, oracle, geo):
    bw, bh = geo[:2]
    cfg, B = K.geo_cfg(geo), 3
    rig_list = [H.small_rig()[n] for n in SC.W.CAMERA_NAMES]
    full = np.random.default_rng(bw * 1000 + bh).integers(0, 256, (B, bh, bw, 3), dtype=np.uint8)
    pool, seen = Pool(ffi), set()
    try:
        d_full, d_full1 = pool.put(full), pool.put(full, 1)
        d_packed = pool.new(B * bw * bh * 3 + 256)
        for blend in (False, True):
            for cams in PACK_CAMS:
                e = hip_engine(cfg, rig_list, cams, blend, False)
                try:
                    x0, y0, x1, y1 = box = e.box
                    if len(cams) == 1:
                        assert box == K.BOXES[geo][blend][cams[0]]
                    if box in seen:
                        continue
                    seen.add(box)
                    want = np.ascontiguousarray(full[:, y0:y1, x0:x1])
                    for vname, src, off in (("aligned", d_full, 0), ("d_full + 1", d_full1, 0), ("d_packed + 1", d_full, 1)):
                        what = "%s, cameras %s blend %d, box %s, %s" % (K.geo_name(geo), cams, blend, box, vname)
                        got = run_into_sentinel(ffi, e.h, d_packed, off, want.nbytes,
                                                lambda p: ffi.lib().bevw_shard_pack_device(e.h, src, B, p), what)
                        H.assert_equal(got.reshape(want.shape), want, what)
                finally:
                    e.close()
    finally:
        pool.free()
    assert len(seen) >= 5, seen   # the four single cameras' boxes differ, and all four cameras own the whole BEV


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_handle_usable(ffi, SB, oracle):
    bw, bh = H.SMALL_CFG["BEV_WIDTH"], H.SMALL_CFG["BEV_HEIGHT"]
    B, img = 2, bw * bh * 3
    L = ffi.lib()
    handles = synth_handles(SB, bw, bh)
    pool = Pool(ffi)
    try:
        d_out = pool.new((B + 1) * img)
        box = (8, 4, 40, 20)
        part = K.fill_parts([box], "random", 1)[0][:B]
        d_part = pool.put(part)
        car = K.make_car(bw, bh, "random")
        d_car = pool.put(car)

        def untouched(status, what):
            assert status == -1, "%s: returned %d" % (what, status)
            assert L.bevw_last_error(), what
            ffi.check(L.bevw_sync(h))
            assert (d_out.download((d_out.nbytes,)) == FILL).all(), what + ": the refused call wrote"

        for kind, (_, h, balance) in handles.items():
            d_out.fill(FILL)
            untouched(combine_call(ffi, h, [], [], B, d_car, d_out.ptr), kind + ": 0 parts")
            untouched(combine_call(ffi, h, [d_part] * 9, [box] * 9, B, d_car, d_out.ptr), kind + ": 9 parts")
            untouched(combine_call(ffi, h, [d_part, None], [box] * 2, B, d_car, d_out.ptr), kind + ": a null part")
            for bad, why in (((40, 4, 40, 20), "x1 == x0"), ((40, 4, 8, 20), "x1 < x0"), ((8, 20, 40, 20), "y1 == y0"), ((8, 4, bw + 1, 20), "x1 > bw"),
                             ((8, 4, 40, bh + 1), "y1 > bh"), ((-4, 4, 28, 20), "negative x0"), ((8, -1, 40, 15), "negative y0")):
                untouched(combine_call(ffi, h, [d_part, d_part], [box, bad], B, d_car, d_out.ptr), "%s: a box with %s" % (kind, why))
            # the handle still combines
            got = run_into_sentinel(ffi, h, d_out, 0, B * img, lambda p: combine_call(ffi, h, [d_part] * 8, [box] * 8, B, d_car, p), kind + " after the refusals")
            H.assert_equal(got.reshape(B, bh, bw, 3), K.combine_statement([part] * 8, [box] * 8, bw, bh, car, balance), kind + " after the refusals")

        # bevw_shard_run_device on a balance shard without V sums; then with them, against the oracle's part
        e, h = handles["balance"][0], handles["balance"][1]
        frames = SC.frames(batch=B)
        d_frames = pool.put(frames)
        d_out.fill(FILL)
        untouched(L.bevw_shard_run_device(h, d_frames, B, None, d_out.ptr), "shard run on a balance shard without V sums")
        orc = K.OracleShards(H.small_rig(), H.SMALL_CFG, frames, True, True)
        H.assert_equal(e.partial(frames, orc.all_vsums), orc.part((0, 1, 2, 3)), "the balance shard after the refusal")
        # bevw_shard_pack_device on a handle that is no shard
        h = handles["blend"][1]
        untouched(L.bevw_shard_pack_device(h, d_part, 1, d_out.ptr), "pack on a handle that is no shard")
        untouched(L.bevw_shard_vsums_device(h, d_frames, B, d_out.ptr), "shard V sums on a handle that is no shard")
        got = handles["blend"][0].batch(frames, car)
        ref = oracle.RefBevGenerator(H.small_rig(), H.SMALL_CFG, blend=True)
        H.assert_equal(got, np.stack([ref(*fs, car=car) for fs in frames]), "the full handle after the refusals")
    finally:
        pool.free()
        for o, _, _ in handles.values():
            (o.close if hasattr(o, "close") else o._engine.close)()
