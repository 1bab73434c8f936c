"""Worker of tests/test_far_batches_gpu.py: one fresh process per case of tests/_far_batches.py, so that every case has a time limit of its own
and the gigabytes of one case are gone before the next starts.

argv: case_file case_name.  case_file (written by the parent) holds the pool of 7 frame sets in the case's input format, the car sprite, the
oracle's 7 expected images in the case's output format and the mask of pixels no camera covers.  The worker derives the batch and every
straddler index from the handle's own in_set_bytes / out_image_bytes, repeats the pool over the batch on the device, fills the output and
one guard image behind it with 0x5A, runs ONE step through the device-resident entry point and compares, at tolerance 0, the images
tests/_far_batches.checked names -- each with the reason it is looked at -- and the guard image.  It prints the wall times of its stages.
The one-channel cases (grey stitch, 8- and 16-bit remappers, linear and nearest) compare planes through tests/_harness.check_plane; the moving
case gets the seven rigs' matrices in case_file too and overwrites its matrix array with NaN as soon as the call returns.

If bevw_malloc itself returns BEVW_E_NOMEM the worker prints a `SKIPPED:` line with the size and ends; nothing else may skip."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import _caller_maps as CM  # noqa: E402
from tests import _far_batches as FB  # noqa: E402
from tests import _harness as H  # noqa: E402

BEVW_E_NOMEM = -4
UPLOAD_BYTES = 256 << 20   # the pool goes up in pieces of whole pools of about this size


class NoMemory(Exception):
    pass


def allocate(ffi, nbytes):
    """A DeviceBuffer, or NoMemory when bevw_malloc returns BEVW_E_NOMEM (every other failure raises as usual)."""
    d = ffi.DeviceBuffer.__new__(ffi.DeviceBuffer)
    d.device, d.nbytes, d.ptr = 0, int(nbytes), None
    p = C.c_void_p()
    status = ffi.lib().bevw_malloc(0, int(nbytes), C.byref(p))
    if status == BEVW_E_NOMEM:
        raise NoMemory("bevw_malloc of %d bytes returned BEVW_E_NOMEM" % nbytes)
    ffi.check(status)
    d.ptr = p.value
    return d


def upload_repeated(d, pool, batch):
    """pool [POOL, ...] repeated over `batch` units of the device buffer, unit b = pool[b % POOL]."""
    unit = pool[0].nbytes
    reps = max(1, UPLOAD_BYTES // pool.nbytes)
    piece = np.ascontiguousarray(np.broadcast_to(pool, (reps,) + pool.shape)).reshape(-1)
    b = 0
    while b < batch:
        n = min(reps * FB.POOL, batch - b)
        d.upload(piece[:n * unit], offset=b * unit)
        b += n


def check_images(d_out, batch, image_bytes, why, compare, name):
    """compare(raw bytes of image b, b % POOL, where): every image `why` names, after the guard image behind the last one."""
    guard = d_out.download((image_bytes,), offset=batch * image_bytes)
    assert (guard == H.FILL).all(), "%s, batch %d: %d bytes of the guard image behind image %d were written (first at byte %d)" % (
        name, batch, int((guard != H.FILL).sum()), batch - 1, int(np.argmax(guard != H.FILL)))
    for b in sorted(why):
        compare(d_out.download((image_bytes,), offset=b * image_bytes), b % FB.POOL, "%s, %s" % (name, FB.where(batch, b, why[b])))


def run_stitch(ffi, SB, c, z):
    cfg, far = FB.GEOMETRIES[c.geometry]
    blend, balance = FB.MODES[c.mode]
    bev = H.generator(SB, FB.scaled_rig(cfg), cfg, blend=blend, balance=balance, input_format=c.inp, output_format=c.out, output_pitch="dense",
                      schedule=ffi.SCHED_PER_PIXEL if c.schedule == "per_pixel" else ffi.SCHED_TILE_PLAN)
    info = bev.plan_info()
    assert c.schedule == "per_pixel" or (info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0), info
    in_unit, out_unit = bev.in_set_bytes, bev.out_image_bytes
    batch = FB.far_batch(in_unit if far == "in" else out_unit)
    stride = FB.stride_for(batch)
    why = FB.checked(batch, in_unit, out_unit, stride, FB.VSUM_CUT if batch * 4 > FB.GRID_MAX else ())
    print("batch %d (%d frames), %d bytes in, %d bytes out, stride %d, %d images checked; straddlers in %s out %s" % (
        batch, batch * 4, batch * in_unit, batch * out_unit, stride, len(why), [FB.straddler(in_unit, x) for x in FB.BOUNDARIES],
        [FB.straddler(out_unit, x) for x in FB.BOUNDARIES]), flush=True)
    pool, car, want, none = z["pool"], z["car"], z["want"], z["none"]
    assert pool[0].nbytes == in_unit and want[0].nbytes == out_unit
    nv12, bw, bh = c.out == "nv12", cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    want_bgr = z["want_bgr"]
    bufs = []
    try:
        t0 = time.time()
        for n in (batch * in_unit, (batch + 1) * out_unit, car.nbytes):
            bufs.append(allocate(ffi, n))
        d_in, d_out, d_car = bufs
        d_out.fill(H.FILL)
        d_car.upload(car)
        upload_repeated(d_in, pool, batch)
        t1 = time.time()
        bev.run_device(d_in.ptr, batch, d_car.ptr, d_out.ptr, out_bytes=batch * out_unit)
        bev.sync()
        t2 = time.time()
        assert bev.last_path() == (ffi.PATH_PER_PIXEL if c.schedule == "per_pixel" else ffi.PATH_UNITS), bev.last_path()

        def compare(raw, k, what):
            H.check_image(H.image_of(raw, nv12, bw, bh, bev.out_pitch), want_bgr[k], none, what, c.out, car=car, want_nv12=want[k] if nv12 else None)

        check_images(d_out, batch, out_unit, why, compare, c.name)
        t3 = time.time()
    finally:
        for d in bufs:
            d.free()
    print("seconds: upload %.2f, step %.2f, check %.2f" % (t1 - t0, t2 - t1, t3 - t2), flush=True)


def run_remap(ffi, c, z):
    far = c.kind == "remap"
    size = FB.REMAP_SIZE if far else FB.COUNT_SIZE
    maps = CM.family(FB.REMAP_FAMILY if far else FB.COUNT_FAMILY, *size)
    pool, want = z["pool"], z["want"]
    in_unit, out_unit = pool[0].nbytes, want[0].nbytes
    batch = FB.far_batch(out_unit) if far else FB.COUNT_BATCH
    stride = FB.stride_for(batch) if far else 1
    why = FB.checked(batch, in_unit, out_unit, stride, range(FB.GRID_MAX - 2, FB.GRID_MAX + 3) if not far else ())
    print("batch %d, %d bytes in, %d bytes out, stride %d, %d images checked; straddlers out %s" % (
        batch, batch * in_unit, batch * out_unit, stride, len(why), [FB.straddler(out_unit, x) for x in FB.BOUNDARIES]), flush=True)
    bufs = []
    try:
        t0 = time.time()
        for n in (batch * in_unit, (batch + 1) * out_unit):
            bufs.append(allocate(ffi, n))
        d_src, d_dst = bufs
        d_dst.fill(H.FILL)
        upload_repeated(d_src, pool, batch)
        t1 = time.time()
        with H.Remapper(ffi, maps, size, "bgr") as r:
            r.remap_device(d_src.ptr, batch, d_dst.ptr)
            t2 = time.time()
            print("remapper path %d" % r.last_path(), flush=True)
            assert far or r.last_path() == ffi.PATH_PER_PIXEL, "BEVW_REMAP_PLAN=0: remap_launch"
        compare = lambda raw, k, what: H.assert_equal(raw.reshape(want[k].shape), want[k], what)
        if not far:   # small images, all of them: one download, and the first image that differs goes to the comparison by name
            raw = d_dst.download((batch, out_unit))
            bad = np.flatnonzero((raw != want.reshape(FB.POOL, out_unit)[np.arange(batch) % FB.POOL]).any(axis=1))
            first = int(bad[0]) if bad.size else batch - 1   # (all equal: the guard image and the last image are still looked at below)
            why = {first: why[first]}
        check_images(d_dst, batch, out_unit, why, compare, c.name)
        t3 = time.time()
    finally:
        for d in bufs:
            d.free()
    print("seconds: upload %.2f, step %.2f, check %.2f" % (t1 - t0, t2 - t1, t3 - t2), flush=True)


def run_stitch_gray(ffi, SB, c, z):
    """BevGenerator(channels=1) on geometry T, direct, dense images: the bases of k_stitch_units_gray / k_stitch_tiles_gray (plan) and the
    cut of gray_stitch_launch_pp (per_pixel) past 2^32 output bytes and past one grid of images."""
    cfg, _ = FB.GEOMETRIES[c.geometry]
    bev = H.generator(SB, FB.scaled_rig(cfg), cfg, channels=1, output_pitch="dense",
                      schedule=ffi.SCHED_PER_PIXEL if c.schedule == "per_pixel" else ffi.SCHED_TILE_PLAN)
    in_unit, out_unit = bev.in_set_bytes, bev.out_image_bytes
    batch = FB.far_batch(out_unit)
    stride = FB.stride_for(batch)
    why = FB.checked(batch, in_unit, out_unit, stride, range(FB.GRID_MAX - 2, FB.GRID_MAX + 3))
    print("batch %d, %d bytes in, %d bytes out, stride %d, %d images checked; straddlers out %s" % (
        batch, batch * in_unit, batch * out_unit, stride, len(why), [FB.straddler(out_unit, x) for x in FB.BOUNDARIES]), flush=True)
    pool, car, want, none = z["pool"], z["car"], z["want"], z["none"]
    assert pool[0].nbytes == in_unit and want[0].nbytes == out_unit and batch > FB.GRID_MAX
    bufs = []
    try:
        t0 = time.time()
        for n in (batch * in_unit, (batch + 1) * out_unit, car.nbytes):
            bufs.append(allocate(ffi, n))
        d_in, d_out, d_car = bufs
        d_out.fill(H.FILL)
        d_car.upload(car)
        upload_repeated(d_in, pool, batch)
        t1 = time.time()
        bev.run_device(d_in.ptr, batch, d_car.ptr, d_out.ptr, out_bytes=batch * out_unit)
        bev.sync()
        t2 = time.time()
        assert bev.last_path() == (ffi.PATH_PER_PIXEL if c.schedule == "per_pixel" else ffi.PATH_UNITS), bev.last_path()
        compare = lambda raw, k, what: H.check_plane(raw.reshape(want[k].shape), want[k], none, what, under=car)
        check_images(d_out, batch, out_unit, why, compare, c.name)
        t3 = time.time()
    finally:
        for d in bufs:
            d.free()
    print("seconds: upload %.2f, step %.2f, check %.2f" % (t1 - t0, t2 - t1, t3 - t2), flush=True)


def run_plane(ffi, c, z):
    """A one-channel remapper (c.depth bits, linear or nearest).  'plane': the far output on the units (2-byte offsets past 2^32);
    'plane_count': 65,540 small images with the plan switched off -- the cut of remap_launch on k_remap_lut_gray16 / k_remap_nn8."""
    from tests import _nearest as N

    far = c.kind == "plane"
    size = FB.REMAP_SIZE if far else FB.COUNT_SIZE
    maps = CM.family(FB.REMAP_FAMILY if far else FB.COUNT_FAMILY, *size)
    pool, want, fixed = z["pool"], z["want"], z["fixed"]
    in_unit, out_unit = pool[0].nbytes, want[0].nbytes
    assert pool.dtype == want.dtype == (np.uint16 if c.depth == 16 else np.uint8)
    batch = FB.far_batch(out_unit) if far else FB.COUNT_BATCH
    stride = FB.stride_for(batch) if far else 1
    why = FB.checked(batch, in_unit, out_unit, stride, range(FB.GRID_MAX - 2, FB.GRID_MAX + 3) if not far else ())
    print("batch %d, %d bytes in, %d bytes out, stride %d, %d images checked; straddlers out %s" % (
        batch, batch * in_unit, batch * out_unit, stride, len(why), [FB.straddler(out_unit, x) for x in FB.BOUNDARIES]), flush=True)
    bufs = []
    try:
        t0 = time.time()
        for n in (batch * in_unit, (batch + 1) * out_unit):
            bufs.append(allocate(ffi, n))
        d_src, d_dst = bufs
        d_dst.fill(H.FILL)
        upload_repeated(d_src, pool.view(np.uint8), batch)
        t1 = time.time()
        with H.Remapper(ffi, maps, size, channels=1) as r:
            N.set_depth(r, c.depth)
            N.set_interpolation(r, c.nearest)
            r.remap_device(d_src.ptr, batch, d_dst.ptr)
            t2 = time.time()
            print("remapper path %d" % r.last_path(), flush=True)
            assert r.last_path() == (ffi.PATH_UNITS if far else ffi.PATH_PER_PIXEL), "far: the units; BEVW_REMAP_PLAN=0: remap_launch"
        compare = lambda raw, k, what: H.check_plane(raw.view(want.dtype).reshape(want[k].shape), want[k], fixed, what)
        if not far:   # small images, all of them: one download, and the first image that differs goes to the comparison by name
            raw = d_dst.download((batch, out_unit))
            bad = np.flatnonzero((raw != want.reshape(FB.POOL, -1).view(np.uint8)[np.arange(batch) % FB.POOL]).any(axis=1))
            first = int(bad[0]) if bad.size else batch - 1
            why = {first: why[first]}
        check_images(d_dst, batch, out_unit, why, compare, c.name)
        t3 = time.time()
    finally:
        for d in bufs:
            d.free()
    print("seconds: upload %.2f, step %.2f, check %.2f" % (t1 - t0, t2 - t1, t3 - t2), flush=True)


def run_moving(ffi, SB, c, z):
    """bevw_run_homographies_device over FB.MOVING_BATCH frame sets, set b on rig b % 7: the launcher's second span starts at set 65535."""
    cfg = FB.MOVING_CFG
    bev = H.generator(SB, FB.scaled_rig(cfg), cfg, output_pitch="dense")
    in_unit, out_unit = bev.in_set_bytes, bev.out_image_bytes
    batch = FB.MOVING_BATCH
    stride = FB.stride_for(batch)
    why = FB.checked(batch, in_unit, out_unit, stride, range(FB.GRID_MAX - 2, FB.GRID_MAX + 3))
    pool, car, want, none, table = z["pool"], z["car"], z["want"], z["none"], z["table"]
    assert pool[0].nbytes == in_unit and want[0].nbytes == out_unit and table.shape == (FB.MOVING_RIGS, 4, 3, 3) and FB.MOVING_RIGS == FB.POOL
    total = batch * in_unit + (batch + 1) * out_unit + car.nbytes
    print("batch %d, %d bytes in, %d bytes out (%d in all), stride %d, %d images checked; straddlers in %s out %s" % (
        batch, batch * in_unit, batch * out_unit, total, stride, len(why), [FB.straddler(in_unit, x) for x in FB.BOUNDARIES],
        [FB.straddler(out_unit, x) for x in FB.BOUNDARIES]), flush=True)
    assert total < 16 << 30
    hs = np.ascontiguousarray(table[np.arange(batch) % FB.MOVING_RIGS])
    bufs = []
    try:
        t0 = time.time()
        for n in (batch * in_unit, (batch + 1) * out_unit, car.nbytes):
            bufs.append(allocate(ffi, n))
        d_in, d_out, d_car = bufs
        d_out.fill(H.FILL)
        d_car.upload(car)
        upload_repeated(d_in, pool, batch)
        t1 = time.time()
        bev.run_homographies_device(d_in.ptr, hs, batch, d_car.ptr, d_out.ptr, out_bytes=batch * out_unit)
        hs[...] = np.nan
        bev.sync()
        t2 = time.time()
        assert bev.last_path() == ffi.PATH_PER_PIXEL, bev.last_path()
        bw, bh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
        compare = lambda raw, k, what: H.check_image(H.image_of(raw, False, bw, bh, bev.out_pitch), want[k], none, what, "bgr", car=car)
        check_images(d_out, batch, out_unit, why, compare, c.name)
        t3 = time.time()
    finally:
        for d in bufs:
            d.free()
    print("seconds: upload %.2f, step %.2f, check %.2f" % (t1 - t0, t2 - t1, t3 - t2), flush=True)


def main():
    case_file, name = sys.argv[1], sys.argv[2]
    c = FB.case(name)
    ffi, SB = H.worker_library(c.env, only=("BEVW_REMAP_PLAN",))
    z = np.load(case_file)
    try:
        if c.kind == "stitch":
            run_stitch(ffi, SB, c, z)
        elif c.kind == "stitch_gray":
            run_stitch_gray(ffi, SB, c, z)
        elif c.kind in ("plane", "plane_count"):
            run_plane(ffi, c, z)
        elif c.kind == "moving":
            run_moving(ffi, SB, c, z)
        else:
            run_remap(ffi, c, z)
    except NoMemory as e:
        print("SKIPPED: %s: %s" % (name, e), flush=True)
    else:
        print("worker OK %s" % name, flush=True)
    print("far worker done", flush=True)


if __name__ == "__main__":
    main()
