"""ONE engine walked through every input layout without being rebuilt (bevw_set_input_format, bevw_set_input_pitch, bevw_set_output_format
and their bevw_remapper_* twins on a live plan), on the GPU.

A plan keeps one pair of group lists per source layout (csrc/bevw_planapi.h: SrcLayout); the lists of a layout are made when a format or
pitch that needs them is first set, and the surface lists again for every new pitch.  The walk below changes the layout nine times on the
same handle and runs one step after every change: BGR, packed NV12, surfaces at pitch FW + 4, surfaces at pitch FW + 64, pitch 0 and packed
NV12 again, YUYV, UYVY, NV12, BGR -- once with BGR images and once with NV12 images, for direct and for blend + balance handles, and on one
fisheye remapper.  A surface list left over from the old pitch, a list made for one layout and read as another, or lists replaced under a
step that is still queued all show as a wrong image: every step is compared with the CPU oracle on the frames the NumPy specifications
(tests/_nv12_spec.py, tests/_yuv422_spec.py) make of its input, NV12 images through tests/_nv12_out_spec.py, with tolerance 0 and the
pixels no camera covers asserted by name.  Every kind of input holds different random bytes, so no two steps expect the same image.
Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests import _nv12_spec as S
from tests import _nv12_surfaces as SF
from tests import _yuv422_spec as Y
from tests._harness import SMALL_CFG as CFG, check_image, ffi, random_car, small_rig, uncovered  # noqa: F401

pytestmark = pytest.mark.gpu

FW, FH, BW, BH = CFG["FRAME_WIDTH"], CFG["FRAME_HEIGHT"], CFG["BEV_WIDTH"], CFG["BEV_HEIGHT"]
BATCH = 3
# (input kind, input pitch of the surfaces): one step after every change
WALK = (("bgr", 0), ("nv12", 0), ("surfaces", FW + 4), ("surfaces", FW + 64), ("nv12", 0), ("yuyv", 0), ("uyvy", 0), ("nv12", 0), ("bgr", 0))


def make_inputs(rng, cams):
    """Random frames of every kind, [BATCH, cams, ...], and the BGR frames the specifications make of them."""
    raw = {"bgr": rng.integers(0, 256, (BATCH, cams, FH, FW, 3), dtype=np.uint8), "nv12": S.random_nv12(rng, (BATCH, cams), FW, FH),
           "yuyv": Y.random_yuv422(rng, (BATCH, cams), FW, FH), "uyvy": Y.random_yuv422(rng, (BATCH, cams), FW, FH)}
    bgr = {"bgr": raw["bgr"], "nv12": np.stack([[S.nv12_to_bgr(f) for f in s] for s in raw["nv12"]]),
           "yuyv": Y.yuv422_to_bgr(raw["yuyv"], "yuyv"), "uyvy": Y.yuv422_to_bgr(raw["uyvy"], "uyvy")}
    return raw, bgr


class Walker:
    """The device side of a walk: the packed inputs, the surfaces at both pitches and the output buffer of one engine; set_* / run_* are the
    engine's C entry points (a handle's or a remapper's)."""

    def __init__(self, ffi, raw, cams, out_bytes, set_format, set_pitch, run_packed, run_surfaces):
        self.ffi, self.cams = ffi, cams
        self.set_format, self.set_pitch, self.run_packed, self.run_surfaces = set_format, set_pitch, run_packed, run_surfaces
        self.packed = {k: ffi.DeviceBuffer(v.nbytes).upload(v) for k, v in raw.items()}
        nv = raw["nv12"].reshape(BATCH * cams, FH * 3 // 2, FW)
        self.surf = {p: SF.Surfaces(ffi, nv, FW, FH, p, layout_seed=p, fill_seed=p + 1, mode="shuffled") for _, p in WALK if p}
        self.out = ffi.DeviceBuffer(BATCH * out_bytes)
        self.kind = "bgr"

    def step(self, kind, pitch):
        """Changes the engine's input to `kind` (and the pitch) as a caller would, runs one step and leaves the images in self.out."""
        ffi = self.ffi
        fmt = "nv12" if kind == "surfaces" else kind
        if fmt != self.kind:
            ffi.check(self.set_format(ffi.INPUT_FORMATS[fmt]))
            self.kind = fmt
        if fmt == "nv12":
            ffi.check(self.set_pitch(pitch))
        self.out.fill(0x5a)
        if kind == "surfaces":
            ffi.check(self.run_surfaces(ffi.ptr(self.surf[pitch].table), BATCH, self.out.ptr))
        else:
            ffi.check(self.run_packed(self.packed[kind].ptr, BATCH, self.out.ptr))
        return "nv12" if kind == "surfaces" else kind

    def free(self):
        for b in list(self.packed.values()) + [self.out]:
            b.free()
        for s in self.surf.values():
            s.free()


def check_images(walker, sync, nv12_out, shape, want, none, what, black):
    walker.ffi.check(sync())
    if nv12_out:
        got = walker.out.download((BATCH, shape[0] * 3 // 2, shape[1]))
    else:
        got = walker.out.download((BATCH, shape[0], shape[1], 3))
    for b in range(BATCH):
        check_image(got[b], want[b], none, "%s, set %d" % (what, b), "nv12" if nv12_out else "bgr", black)


@pytest.mark.parametrize("blend,balance", [(0, 0), (1, 1)])
def test_one_handle_through_every_input_layout(ffi, oracle, blend, balance):
    L = ffi.lib()
    rng = np.random.default_rng(9100 + blend)
    raw, bgr = make_inputs(rng, 4)
    car = random_car(rng, CFG)
    rig = small_rig()
    ref = oracle.RefBevGenerator(rig, CFG, blend=bool(blend), balance=bool(balance))
    none = uncovered(ref)
    assert none.any()
    want = {k: [ref(*v[b], car) for b in range(BATCH)] for k, v in bgr.items()}   # once per kind of input, shared by the steps
    cfg = ffi.bevw_config(FW, FH, BW, BH, CFG["CAR_WIDTH"], CFG["CAR_HEIGHT"], CFG["FOCAL_SCALE"], CFG["SIZE_SCALE"], blend, balance, 0, ffi.SCHED_AUTO)
    h = C.c_void_p()
    ffi.check(L.bevw_create(C.byref(cfg), C.byref(h)))
    walker = d_car = None
    try:
        for i, n in enumerate(W.CAMERA_NAMES):
            K, D, H = (ffi.f64(m, k) for m, k in zip(rig[n], (9, 4, 9)))   # (held until the call returns)
            ffi.check(L.bevw_set_camera(h, i, ffi.ptr(K), ffi.ptr(D), ffi.ptr(H)))
        ffi.check(L.bevw_build(h))
        info = np.zeros(8, np.int32)
        ffi.check(L.bevw_plan_info(h, ffi.ptr(info)))
        assert info[2] == ffi.SCHED_TILE_PLAN and info[5] > 0   # the units run: their group lists are what the walk is about
        assert L.bevw_output_pitch(h) == BW
        d_car = ffi.DeviceBuffer(car.nbytes).upload(car)
        walker = Walker(ffi, raw, 4, BW * BH * 3,
                        lambda f: L.bevw_set_input_format(h, f), lambda p: L.bevw_set_input_pitch(h, p),
                        lambda d, n, o: L.bevw_run_device(h, d, n, d_car.ptr, o), lambda t, n, o: L.bevw_run_surfaces_device(h, t, n, d_car.ptr, o))
        for out_fmt in (ffi.OUTPUT_BGR, ffi.OUTPUT_NV12):
            ffi.check(L.bevw_set_output_format(h, out_fmt))
            for k, (kind, pitch) in enumerate(WALK):
                frames = walker.step(kind, pitch)
                assert L.bevw_input_pitch(h) == (pitch or FW)
                what = "blend %d balance %d, %s images, step %d: %s%s" % (blend, balance, "NV12" if out_fmt else "BGR", k + 1, kind, " at pitch %d" % pitch if pitch else "")
                check_images(walker, lambda: L.bevw_sync(h), out_fmt == ffi.OUTPUT_NV12, (BH, BW), want[frames], none, what, black=False)
    finally:
        if walker:
            walker.free()
        if d_car:
            d_car.free()
        L.bevw_destroy(h)


def test_one_remapper_through_every_input_layout(ffi, oracle):
    L = ffi.lib()
    rng = np.random.default_rng(9200)
    raw, bgr = make_inputs(rng, 1)
    K, D, _ = small_rig()["front"]
    r = C.c_void_p()
    K9, D4 = ffi.f64(K, 9), ffi.f64(D, 4)   # (held until the call returns)
    ffi.check(L.bevw_fisheye_remapper_create(0, FW, FH, ffi.ptr(K9), ffi.ptr(D4), 1.0, 1.0, 0.0, 0.0, C.byref(r)))
    walker = None
    try:
        dims = np.zeros(4, np.int32)
        ffi.check(L.bevw_remapper_dims(r, ffi.ptr(dims)))
        dw, dh = int(dims[2]), int(dims[3])
        assert (dw, dh) == (FW, FH)
        m1, m2 = np.empty((dh, dw, 2), np.int16), np.empty((dh, dw), np.uint16)
        ffi.check(L.bevw_remapper_get_maps(r, ffi.ptr(m1), ffi.ptr(m2)))
        o1, o2 = oracle.fisheye_init_undistort_rectify_map(K, D, oracle.camera_mat_dst(K, FW, FH, 1.0, 1.0), (dw, dh))
        assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
        outside = (m1[..., 0] < -1) | (m1[..., 0] >= FW) | (m1[..., 1] < -1) | (m1[..., 1] >= FH)
        want = {k: [oracle.remap(v[b, 0], o1, o2) for b in range(BATCH)] for k, v in bgr.items()}
        walker = Walker(ffi, raw, 1, dw * dh * 3,
                        lambda f: L.bevw_remapper_set_input_format(r, f), lambda p: L.bevw_remapper_set_input_pitch(r, p),
                        lambda d, n, o: L.bevw_remap_device(r, d, n, o), lambda t, n, o: L.bevw_remap_surfaces_device(r, t, n, o))
        for out_fmt in (ffi.OUTPUT_BGR, ffi.OUTPUT_NV12):
            ffi.check(L.bevw_remapper_set_output_format(r, out_fmt))
            for k, (kind, pitch) in enumerate(WALK):
                frames = walker.step(kind, pitch)
                what = "remapper, %s images, step %d: %s%s" % ("NV12" if out_fmt else "BGR", k + 1, kind, " at pitch %d" % pitch if pitch else "")
                check_images(walker, lambda: L.bevw_remapper_sync(r), out_fmt == ffi.OUTPUT_NV12, (dh, dw), want[frames], outside, what, black=True)
    finally:
        if walker:
            walker.free()
        L.bevw_remapper_destroy(r)
