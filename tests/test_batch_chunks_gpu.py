"""The batch loop of the plan kernels on the GPU: ragged chunks, frames per block of 2 and 3, XCD-affine launches whose chunk count is no
multiple of 8, balance slices with a chunk size of their own -- in every pixel format, on every unit kernel (k_plan_units x 4,
k_units_nv12, k_units_out_nv12, k_units_surf, k_units_out_surf, k_plan_unit_wide) and the one-camera remapper plan.

plan_args (csrc/bevw_plan.h) cuts a batch into chunks of nb frames; a block of plan_unit_run (csrc/bevw_unit.h) keeps two frames of group
loads in flight and steps its chunk by two, so a chunk of odd length runs one step past its end: frame_of() clamps that step to the
chunk's last frame.  A clamp that is wrong by one writes a chunk's last frame into the NEXT chunk's first image and races its rightful
writer.  The batch sizes here -- BATCHES, in an order that first shrinks and then grows every scratch buffer of a handle -- were chosen by
the table below (PLAIN, SLICES); tests/test_batch_map_host.py asserts that table against the library's own plan_args, so a change of the
nb heuristic flags this list as stale.

Every frame set of a batch is distinct and uniform random, every run has the car sprite, and every image of every batch is compared with
tolerance 0 against the CPU oracle (oracle.RefBevGenerator, oracle.remap) on the _nv12_spec-converted frames (NV12 images: through
_nv12_out_spec).  The expected images are computed once per module; an image that differs from them goes to assert_same / assert_nv12 of
the NV12 modules, which name the pixels no camera covers first.  Before each run the whole output buffer -- one image larger than the
largest batch -- is filled with 0x5A: the frames at a position are the same from run to run, so a stale image would otherwise pass, and
the image-sized guard behind image B - 1 must still hold the fill afterwards.  (Padding columns inside an image are not asserted: units
may own them.)  Run with `-m gpu` on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _nv12_out_spec as SO
from tests import _nv12_spec as S
from tests import _nv12_surfaces as SF
from tests import test_nv12_gpu as TI
from tests import test_nv12_out_gpu as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = TI.SMALL_CFG
POOL = 143                                     # distinct frame sets; a batch of B is the first B of them
BATCHES = (143, 9, 63, 17, 129, 31, 100, 33)   # in this order on one handle
FILL = 0x5A
MODES = ((False, False), (True, False), (False, True), (True, True))   # (blend, balance)
# batch -> (nb, chunks, frames of the last chunk, XCD map in use, idle chunk slots of the launch) without balance slices ...
PLAIN = {9: (1, 9, 1, 1, 7), 17: (2, 9, 1, 1, 7), 31: (3, 11, 1, 1, 5), 33: (8, 5, 1, 0, 0), 63: (8, 8, 7, 1, 0), 100: (8, 13, 4, 1, 3),
         129: (16, 9, 1, 1, 7), 143: (16, 9, 15, 1, 7)}
# ... and the slices of a balance handle (balance_plan_run, csrc/bevwarp.hip: two from batch 32), each (frames, nb, chunks, last chunk)
SLICES = {9: ((9, 1, 9, 1),), 17: ((17, 2, 9, 1),), 31: ((31, 3, 11, 1),), 33: ((16, 2, 8, 2), (17, 2, 9, 1)),
          63: ((31, 3, 11, 1), (32, 8, 4, 8)), 100: ((50, 8, 7, 2), (50, 8, 7, 2)), 129: ((64, 8, 8, 8), (65, 8, 9, 1)),
          143: ((71, 8, 9, 7), (72, 8, 9, 8))}


def balance_slices(batch):
    """Frame sets per slice of a balance handle's step, as balance_plan_run cuts them."""
    parts = 2 if batch >= 32 else 1
    return [batch * (p + 1) // parts - batch * p // parts for p in range(parts)]


def where(batch, b, balance=False, nb_env=0):
    """'batch B, frame b: chunk c of n frames, last of its chunk or not' -- with the table's nb (nb_env: an explicit BEVW_PLAN_NB)."""
    slices = [(n, nb) for n, nb, _, _ in SLICES[batch]] if balance else [(batch, PLAIN[batch][0])]
    b0 = 0
    for k, (n, nb) in enumerate(slices):
        nb = min(nb_env, n) if nb_env else nb
        if b < b0 + n:
            i = b - b0
            last = i % nb == nb - 1 or i == n - 1
            return "batch %d, frame %d: %schunk %d (%d frames per chunk), %s of its chunk" % (
                batch, b, "slice %d of %d frames, " % (k, n) if len(slices) > 1 else "", i // nb, nb, "the LAST frame" if last else "not the last frame")
        b0 += n
    raise AssertionError((batch, b))


@pytest.fixture(scope="module")
def ffi():
    from cameracalibration_amd import _ffi

    _ffi.require_device()
    return _ffi


@pytest.fixture(scope="module")
def SB():
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV

    return surroundBEV


# ---------------------------------------------------------------------------------------------------------------
# inputs and expected images, once per module
# ---------------------------------------------------------------------------------------------------------------
def make_pool(n=POOL, seed=5100):
    """n distinct uniform random NV12 frame sets, the BGR frames the input specification makes of them, and a car sprite."""
    fw, fh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]
    rng = np.random.default_rng(seed)
    nv = S.random_nv12(rng, (n, 4), fw, fh)
    bgr = np.stack([S.nv12_to_bgr(nv[b]) for b in range(n)])
    return nv, bgr, TI.random_car(rng, CFG)


@pytest.fixture(scope="module")
def pool():
    return make_pool()


class Expected:
    """The oracle's images of the pool's frame sets per (blend, balance), computed on first use: .bgr [n, BH, BW, 3], .nv12, .none."""

    def __init__(self, oracle, bgr, car, cfg=CFG, n=POOL, nv12=True):
        self.oracle, self.frames, self.car, self.cfg, self.n, self.with_nv12, self.cache = oracle, bgr, car, cfg, n, nv12, {}

    def __call__(self, blend, balance):
        key = (bool(blend), bool(balance))
        if key not in self.cache:
            ref = self.oracle.RefBevGenerator(TI.small_rig(), self.cfg, blend=key[0], balance=key[1])
            none = TI.uncovered(ref)
            assert none.any()
            want = np.stack([ref(*self.frames[b], self.car) for b in range(self.n)])
            nv12 = np.stack([SO.bgr_to_nv12(w) for w in want]) if self.with_nv12 else None
            self.cache[key] = (want, nv12, none)
        return self.cache[key]


@pytest.fixture(scope="module")
def expected(oracle, pool):
    return Expected(oracle, pool[1], pool[2])


class Inputs:
    """The pool resident on the device once per input kind: packed BGR, packed NV12, NV12 surfaces at pitch FW + 4 with their table, and
    (yuv422: {'yuyv': frames, 'uyvy': frames}) the packed 4:2:2 forms of a pool that has them."""

    def __init__(self, ffi, nv, bgr, car, cams=4, yuv422=None):
        self.ffi, self.nv, self.bgr, self.cams, self.bufs, self.surf, self.yuv422 = ffi, nv, bgr, cams, {}, None, yuv422 or {}
        self.car = ffi.DeviceBuffer(car.nbytes).upload(car) if car is not None else None

    def host(self, kind):
        return self.bgr if kind == "bgr" else self.yuv422[kind] if kind in self.yuv422 else self.nv

    def packed(self, kind):
        if kind not in self.bufs:
            host = self.host(kind)
            self.bufs[kind] = self.ffi.DeviceBuffer(host.nbytes).upload(host)
        return self.bufs[kind]

    def table(self):
        if self.surf is None:
            fw, fh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]
            self.surf = SF.Surfaces(self.ffi, self.nv.reshape(-1, fh * 3 // 2, fw), fw, fh, fw + 4, layout_seed=51, fill_seed=52, mode="shuffled")
            self.bufs["table"] = self.ffi.DeviceBuffer(self.surf.table.nbytes).upload(self.surf.table)
        return self.bufs["table"]

    def free(self):
        for d in self.bufs.values():
            d.free()
        if self.surf is not None:
            self.surf.free()
        if self.car is not None:
            self.car.free()


@pytest.fixture(scope="module")
def inputs(ffi, pool):
    i = Inputs(ffi, pool[0], pool[1], pool[2])
    yield i
    i.free()


# ---------------------------------------------------------------------------------------------------------------
# one handle over a list of batch sizes (also the worker's: tests/_batch_chunks_worker.py)
# ---------------------------------------------------------------------------------------------------------------
def image_of(raw, nv12, bw, bh, pitch):
    """One device image (flat bytes, rows of `pitch` pixels) -> dense BGR [bh, bw, 3] or NV12 [bh * 3 // 2, bw]."""
    return raw.reshape(bh * 3 // 2, pitch)[:, :bw] if nv12 else raw.reshape(bh, pitch, 3)[:, :bw]


def first_difference(got, want):
    at = np.argwhere(got != want)[0].tolist()
    return "first difference at %s: got %d, want %d" % (at, int(got[tuple(at)]), int(want[tuple(at)]))


def check_image(got, want_bgr, want_nv12, none, nv12, what, black=False):
    """Tolerance 0.  An image that differs goes to the NV12 modules' assertions: the pixels no camera covers first, by name."""
    want = want_nv12 if nv12 else want_bgr
    if got.shape == want.shape and np.array_equal(got, want):
        return
    what = "%s; %s" % (what, first_difference(got, want) if got.shape == want.shape else "shape %s" % (got.shape,))
    if nv12:
        TO.assert_nv12(got, want_bgr, none, what, black=black)
    else:
        TI.assert_same(got, want_bgr, none, what)
    raise AssertionError(what)


def run_batches(ffi, launch, sync, image_bytes, nv12, bw, bh, pitch, batches, want, what, balance=False, nb_env=0, black=False):
    """launch(B, d_out) enqueues a step over the first B frame sets into d_out; every image of every batch against want = (bgr, nv12, none),
    the sentinel fill before and the guard image after each run."""
    want_bgr, want_nv12, none = want
    d_out = ffi.DeviceBuffer((max(batches) + 1) * image_bytes)
    try:
        for B in batches:
            d_out.fill(FILL)
            launch(B, d_out)
            sync()
            raw = d_out.download((B + 1, image_bytes))
            assert (raw[B] == FILL).all(), "%s, batch %d: %d bytes of the guard image behind image %d were written (first at byte %d)" % (
                what, B, int((raw[B] != FILL).sum()), B - 1, int(np.argmax(raw[B] != FILL)))
            for b in range(B):
                check_image(image_of(raw[b], nv12, bw, bh, pitch), want_bgr[b], want_nv12[b] if nv12 else None, none, nv12,
                            "%s, %s" % (what, where(B, b, balance, nb_env)), black)
    finally:
        d_out.free()


def stitch_handle(ffi, SB, inputs, want, inp, out, blend, balance, batches=BATCHES, cfg=CFG, nb_env=0, host_entry=True, one_slice=False, **kw):
    """One BevGenerator over `batches` through the device-resident entry, then (packed handles) the host entry on 17 sets in reversed order.
    inp: 'bgr', 'nv12', 'surfaces', or 'yuyv' / 'uyvy' where `inputs` has those forms.  one_slice: a balance handle that does not cut its
    step into slices (the plan's padded scratch), for the position a failure names."""
    fw = cfg["FRAME_WIDTH"]
    what = "%s -> %s, blend %d balance %d" % (inp, out, blend, balance)
    kw = dict(dict(blend=blend, balance=balance, input_format=inp if inp in ("bgr",) + tuple(inputs.yuv422) else "nv12", output_format=out), **kw)
    if inp == "surfaces":
        kw["input_pitch"] = fw + 4
    bev = TI.generator(SB, TI.small_rig(), cfg, **kw)
    info = bev.plan_info()
    assert info["schedule"] == ffi.SCHED_TILE_PLAN and info["tiles_staged"] > 0, what   # the unit kernels run
    car = inputs.car.ptr
    if inp == "surfaces":
        d_table = inputs.table()
        launch = lambda B, d_out: bev.run_surface_table(d_table.ptr, B, car, d_out.ptr, out_bytes=d_out.nbytes)
    else:
        d_in = inputs.packed(inp)
        assert bev.in_set_bytes * inputs.nv.shape[0] == d_in.nbytes
        launch = lambda B, d_out: bev.run_device(d_in.ptr, B, car, d_out.ptr, out_bytes=d_out.nbytes)
    nv12 = out == "nv12"
    run_batches(ffi, launch, bev.sync, bev.out_image_bytes, nv12, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], bev.out_pitch, batches, want, what,
                balance=balance and not one_slice, nb_env=nb_env)
    if host_entry and inp != "surfaces":
        host = inputs.host(inp)
        car_host = inputs.car.download(want[0][0].shape)
        got = bev.batch(host[:17][::-1], car_host)
        for i in range(17):
            check_image(got[i], want[0][16 - i], want[1][16 - i] if nv12 else None, want[2], nv12,
                        "%s, host entry, reversed: position %d = set %d; %s" % (what, i, 16 - i, where(17, i, balance and not one_slice, nb_env)))
    return bev


# ---------------------------------------------------------------------------------------------------------------
# 1. every input kind x output format x (blend, balance): one handle per case, the eight batch sizes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend,balance", MODES)
@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("inp", ["bgr", "nv12", "surfaces"])
def test_ragged_batches_match_oracle(ffi, SB, inputs, expected, inp, out, blend, balance):
    bev = stitch_handle(ffi, SB, inputs, expected(blend, balance), inp, out, blend, balance)
    assert bev.out_pitch == 256   # 'auto': rows of whole 64-byte sectors


@pytest.mark.parametrize("blend,balance", [(False, False), (True, True)])
def test_ragged_batches_dense_layout(ffi, SB, inputs, expected, blend, balance):
    bev = stitch_handle(ffi, SB, inputs, expected(blend, balance), "bgr", "bgr", blend, balance, output_pitch="dense")
    assert bev.out_pitch == CFG["BEV_WIDTH"]


def test_ragged_batches_padded_scratch(ffi, SB, oracle, pool, inputs):
    """A BEV width that is no multiple of 4 with dense images: the units write rows of 252 pixels into the plan's padded scratch, which grows
    with the first batch and is reused by the smaller ones, and k_plan_unpad compacts them."""
    cfg = dict(CFG, BEV_WIDTH=250)
    car = TI.random_car(np.random.default_rng(5250), cfg)
    want_bgr, _, none = Expected(oracle, pool[1], car, cfg, 63, nv12=False)(True, False)
    padded = Inputs(ffi, pool[0], pool[1], car)
    padded.bufs["bgr"] = inputs.packed("bgr")
    try:
        bev = stitch_handle(ffi, SB, padded, (want_bgr, None, none), "bgr", "bgr", True, False, batches=(63, 9, 31), cfg=cfg, output_pitch="dense")
        assert bev.out_pitch == 250
    finally:
        padded.car.free()


# ---------------------------------------------------------------------------------------------------------------
# 2. the fisheye undistorter of the front camera: the one-camera plan, 320 x 256 frames -> 640 x 512 images
# ---------------------------------------------------------------------------------------------------------------
UND_POOL, UND_BATCHES = 100, (100, 9, 63, 17, 31)


@pytest.fixture(scope="module")
def und_case(ffi, oracle, pool):
    fw, fh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]
    nv, bgr = np.ascontiguousarray(pool[0][:UND_POOL, 0]), np.ascontiguousarray(pool[1][:UND_POOL, 0])
    K, D, _ = TI.small_rig()["front"]
    size = (int(fw * CFG["SIZE_SCALE"]), int(fh * CFG["SIZE_SCALE"]))
    o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, oracle.camera_mat_dst(K, fw, fh, CFG["FOCAL_SCALE"], CFG["SIZE_SCALE"]), size)
    outside = (o1[..., 0] < -1) | (o1[..., 0] >= fw) | (o1[..., 1] < -1) | (o1[..., 1] >= fh)
    want = np.stack([oracle.remap(f, o1, o2) for f in bgr])
    assert want.shape[1:] == (512, 640, 3)
    dev = Inputs(ffi, nv, bgr, None, cams=1)
    yield dev, (want, np.stack([SO.bgr_to_nv12(w) for w in want]), outside)
    dev.free()


@pytest.mark.parametrize("out", ["bgr", "nv12"])
@pytest.mark.parametrize("inp", ["bgr", "nv12", "surfaces"])
def test_undistorter_ragged_batches(ffi, und_case, inp, out):
    from cameracalibration_amd.Tools import undistort as U

    dev, want = und_case
    fw, fh = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"]
    K, D, _ = TI.small_rig()["front"]
    und = U.Undistorter(K, D, fw, fh, focalscale=CFG["FOCAL_SCALE"], sizescale=CFG["SIZE_SCALE"], input_format="bgr" if inp == "bgr" else "nv12",
                        output_format=out, input_pitch=fw + 4 if inp == "surfaces" else None)
    try:
        assert (und.out_w, und.out_h) == (640, 512)
        L = ffi.lib()
        if inp == "surfaces":
            d_table = dev.table()
            launch = lambda B, d_out: und.run_surface_table(d_table.ptr, B, d_out.ptr, out_bytes=d_out.nbytes)
        else:
            d_in = dev.packed(inp)
            launch = lambda B, d_out: ffi.check(L.bevw_remap_device(und._r, d_in.ptr, B, d_out.ptr))
        run_batches(ffi, launch, und.sync, und.out_image_bytes, out == "nv12", und.out_w, und.out_h, und.out_w, UND_BATCHES, want,
                    "undistort %s -> %s" % (inp, out), black=True)
    finally:
        und.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. the analytic projection (k_plan_unit_wide): every image of a batch = what the same handle returns for that frame set alone
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [False, True])
def test_analytic_batches_equal_single_frames(ffi, SB, inputs, blend):
    """Batch 1 is anchored to the fp64 specification of the mode by tests/test_analytic.py; the arithmetic per frame does not depend on the
    batch, so any difference here is the batch loop of k_plan_unit_wide."""
    bev = TI.generator(SB, TI.small_rig(), CFG, blend=blend, projection="analytic")
    bw, bh = CFG["BEV_WIDTH"], CFG["BEV_HEIGHT"]
    assert bev.out_pitch == bw and bev.out_image_bytes == bw * bh * 3
    d_in, car, img = inputs.packed("bgr"), inputs.car.ptr, bev.out_image_bytes
    d_one = ffi.DeviceBuffer(34 * img)
    try:
        d_one.fill(FILL)
        for b in range(33):
            bev.run_device(d_in.ptr + b * bev.in_set_bytes, 1, car, d_one.ptr + b * img, out_bytes=img)
        bev.sync()
        alone = d_one.download((34, bh, bw, 3))
    finally:
        d_one.free()
    assert (alone[33] == FILL).all() and all((alone[b] != FILL).any() for b in range(33))
    assert not np.array_equal(alone[0], alone[1])
    none = np.zeros((bh, bw), bool)
    launch = lambda B, d_out: bev.run_device(d_in.ptr, B, car, d_out.ptr, out_bytes=d_out.nbytes)
    run_batches(ffi, launch, bev.sync, img, False, bw, bh, bw, (17, 33), (alone, None, none), "analytic, blend %d" % blend)


# ---------------------------------------------------------------------------------------------------------------
# 4. the launch-map switches, each in a fresh child (the library reads BEVW_PLAN_* once per process)
# ---------------------------------------------------------------------------------------------------------------
SWITCHES = {"xcdmap2": ("BEVW_PLAN_XCDMAP", "2"), "xcdmap0": ("BEVW_PLAN_XCDMAP", "0"), "nb5": ("BEVW_PLAN_NB", "5")}
WORKER_BATCHES = (143, 17, 63)
WORKER_MODES = ((False, False), (True, False), (True, True))   # packed BGR in, BGR out; and surfaces -> NV12 in the blend mode
CHILD_TIMEOUT = 180   # seconds: a library load, four small handles and their steps take a few seconds


@pytest.fixture(scope="module")
def case_dir(pool, expected, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_chunks"))
    nv, bgr, car = pool
    files = dict(nv=nv, bgr=bgr, car=car)
    for m, (blend, balance) in enumerate(WORKER_MODES):
        want, nv12, none = expected(blend, balance)
        files["want%d" % m], files["none%d" % m] = want, none
        if (blend, balance) == (True, False):
            files["want_nv12_%d" % m] = nv12
    for name, a in files.items():
        np.save(os.path.join(d, name + ".npy"), a)
    return d


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_launch_map_switches(case_dir, switch):
    worker = os.path.join(ROOT, "tests", "_batch_chunks_worker.py")
    name, value = SWITCHES[switch]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BEVW_PLAN_")}
    env[name] = value
    p = subprocess.run([sys.executable, worker, case_dir, name, value], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(p.stdout)
    assert p.returncode == 0, "%s=%s: worker exit %d\n%s\n%s" % (name, value, p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    assert "worker OK %s=%s" % (name, value) in p.stdout
