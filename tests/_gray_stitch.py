"""What the tests of the one-channel stitch share (BevGenerator(channels=1), bevw_set_channels): the specification in NumPy over the
committed oracle, the inputs of the small rig, the file interface of tests/native/gray_stitch_emulate.cpp, and the device-side runner of
the GPU cases.  Imported as `tests._gray_stitch`; the library is loaded inside the functions that need it."""
import struct
import subprocess

import numpy as np

from tests import _harness as H


# ---------------------------------------------------------------------------------------------------------------
# the specification: the reference's __call__ with its cv2 calls made on (H, W) arrays
# ---------------------------------------------------------------------------------------------------------------
def spec(oracle, ref, frames4, car=None):
    """frames4: four uint8 (FH, FW) arrays (front, back, left, right); ref: the RefBevGenerator of the rig (its maps and masks; no balance);
    car: uint8 (BH, BW) or None.  cv2.remap per camera, the mask (direct: bitwise_and -- where(m != 0, v, 0); blend: trunc(f32(v) *
    f32(m / 255.0))), cv2.add in camera order, then the car."""
    assert not ref.balance
    parts = []
    for img, cam, m in zip(frames4, ref.cameras, ref.masks):
        assert img.ndim == 2 and img.dtype == np.uint8
        v = oracle.remap(img, *cam.bev_maps)
        assert v.shape == m.shape and v.dtype == np.uint8
        if ref.blend:
            parts.append((v.astype(np.float32) * (m / 255.0).astype(np.float32)).astype(np.uint8))
        else:
            parts.append(np.where(m != 0, v, 0).astype(np.uint8))
    out = parts[0]
    for p in parts[1:]:
        out = oracle.add_sat(out, p)
    if car is not None:
        out = oracle.add_sat(out, car)
    return out


def spec_batch(oracle, ref, frames, car=None):
    """frames uint8 [B, 4, FH, FW] -> [B, BH, BW]"""
    return np.stack([spec(oracle, ref, list(f), car) for f in frames])


def contributors(ref):
    """Per BEV pixel, the number of cameras whose mask is not zero."""
    return np.sum([np.asarray(m) != 0 for m in ref.masks], axis=0)


def gray_frames(rng, cfg, batch, dim=True):
    """Random grey frame sets [batch, 4, FH, FW]; dim: the back camera at half brightness."""
    f = rng.integers(0, 256, (batch, 4, cfg["FRAME_HEIGHT"], cfg["FRAME_WIDTH"]), dtype=np.uint8)
    if dim:
        f[:, 1] //= 2
    return f


def gray_car(rng, cfg):
    """A random grey sprite, centred on a zero canvas of the BEV's size."""
    return np.ascontiguousarray(H.random_car(rng, cfg)[..., 0])


# ---------------------------------------------------------------------------------------------------------------
# tests/native/gray_stitch_emulate.cpp
# ---------------------------------------------------------------------------------------------------------------
def emulate(exe, tmp_path, ref, frames, car, cfg):
    """frames uint8 [n, 4, FH, FW]; the oracle's tables and masks of `ref` -> dict(units, claimed, two, classes, written, img, log)"""
    fw, fh, bw, bh = cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", fw, fh, bw, bh, 4, frames.shape[0], int(car is not None), int(ref.blend)))
        for cam, mk in zip(ref.cameras, ref.masks):
            m1, m2 = cam.bev_maps
            f.write(np.ascontiguousarray(m1, np.int16).tobytes())
            f.write(np.ascontiguousarray(m2, np.uint16).tobytes())
            f.write(np.ascontiguousarray(mk, np.uint8).tobytes())
        f.write(np.ascontiguousarray(frames, np.uint8).tobytes())
        if car is not None:
            f.write(np.ascontiguousarray(car, np.uint8).tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    units, claimed, two, classes = struct.unpack("<4i", raw[:16])
    written = np.frombuffer(raw, np.uint8, bw * bh, 16).reshape(bh, bw)
    img = np.frombuffer(raw, np.uint8, frames.shape[0] * bh * bw, 16 + bw * bh).reshape(frames.shape[0], bh, bw)
    return dict(units=units, claimed=claimed, two=two, classes=classes, written=written, img=img, log=r.stdout)


# ---------------------------------------------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------------------------------------------
FILL = 0x5A


def assert_images(got, want, none, car, what):
    """[B, BH, BW] against the specification at tolerance 0; the pixels no camera covers first: 0, or the car."""
    assert got.shape == want.shape and got.dtype == np.uint8, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    for b in range(got.shape[0]):
        under = got[b][none]
        if car is None:
            assert not under.any(), "%s, image %d: %d pixels no camera covers are not 0" % (what, b, int(np.count_nonzero(under)))
        else:
            assert np.array_equal(under, car[none]), "%s, image %d: pixels no camera covers are not the car" % (what, b)
        H.assert_equal(got[b], want[b], "%s, image %d" % (what, b))


def run_device(ffi, bev, frames, car, batch=None, off_frames=0, off_out=0, off_car=0, check_guards=True):
    """One run_device step on buffers of exactly the batch's bytes between FILL guards (off_*: byte offsets that misalign a buffer) ->
    (images [B, BH, pitch] with the padding columns, the path of the step)."""
    B = frames.shape[0] if batch is None else batch
    c = bev._engine.cfg
    guard = 256
    need = B * bev.out_image_bytes
    d_in = ffi.DeviceBuffer(frames.nbytes + 8)
    d_out = ffi.DeviceBuffer(guard + need + guard + 8)
    d_car = ffi.DeviceBuffer(car.nbytes + 8) if car is not None else None
    try:
        d_in.upload(frames, off_frames)
        if d_car:
            d_car.upload(car, off_car)
        d_out.fill(FILL)
        bev.run_device(d_in.ptr + off_frames, B, d_car.ptr + off_car if d_car else None, d_out.ptr + guard + off_out, out_bytes=need)
        bev.sync()
        raw = d_out.download((guard + need + guard + 8,))
        if check_guards:
            before, after = raw[:guard + off_out], raw[guard + off_out + need:]
            assert (before == FILL).all() and (after == FILL).all(), "bytes outside the batch's %d were written" % need
        return raw[guard + off_out:guard + off_out + need].reshape(B, c.bev_height, bev.out_pitch).copy(), bev.last_path()
    finally:
        d_in.free()
        d_out.free()
        if d_car:
            d_car.free()
