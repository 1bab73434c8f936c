"""What the tests of the stitch with a homography per frame set share (bevw_run_homographies_device, BevGenerator.batch_homographies):
the homography families, the two yardsticks -- A: the committed oracle's RefBevGenerator of the rig with H_b; B: a fresh BevGenerator of
that rig on the library's existing path -- the census on the oracle, and the device-side runner of the GPU cases.  Imported as
`tests._moving`; the library is loaded inside the functions that need it.

A family perturbs every camera's H as a rotation R of the camera does: H_b = H @ inv(Kd R Kd^-1) with Kd = camera_mat_dst(K), the camera
matrix of the undistorted grid H starts from."""
import numpy as np

from tests import _harness as H

CFG = H.SMALL_CFG
CAMERAS = ("front", "back", "left", "right")
FILL = 0x5A


# ---------------------------------------------------------------------------------------------------------------
# homography families
# ---------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def rotated(oracle, K, Hm, cfg, axis, degrees):
    """H of a camera rotated by `degrees` about `axis` (x: pitch, y: yaw, z: roll)."""
    Kd = oracle.camera_mat_dst(K, cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], cfg["FOCAL_SCALE"], cfg["SIZE_SCALE"])
    return Hm @ np.linalg.inv(Kd @ rotation(axis, degrees) @ np.linalg.inv(Kd))


def with_h(rig, f):
    """the rig with H of every camera replaced by f(name, K, H)"""
    return {n: (K, D, np.ascontiguousarray(f(n, K, Hm), np.float64)) for n, (K, D, Hm) in rig.items()}


SMOOTH = (("pitch +0.5", "x", 0.5), ("pitch -2", "x", -2.0), ("yaw 1", "y", 1.0), ("roll 1", "z", 1.0))


def smooth_rigs(oracle, rig, cfg=CFG):
    """[(name, rig)]: every camera pitched by +0.5 and -2 degrees, yawed by 1, rolled by 1"""
    return [(name, with_h(rig, lambda n, K, Hm, ax=ax, deg=deg: rotated(oracle, K, Hm, cfg, ax, deg))) for name, ax, deg in SMOOTH]


def shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def singular(Hm):
    """H with its last row replaced by its second: each of the three cofactors of the first row is a * b - b * a, so the determinant the
    cofactor expansion computes is exactly 0.0"""
    S = np.array(Hm, np.float64)
    S[2] = S[1]
    return S


def hostile_rigs(oracle, rig, cfg=CFG):
    """[(name, rig)]: the rig's own H; a BEV-side shift by 60 pixels; a yaw of 15 degrees; a zoom by 0.5 about the BEV's centre; a singular
    matrix; the front camera alone pitched by -2 degrees"""
    bw, bh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    C = shift(bw / 4.0, bh / 4.0)
    return [("own H", with_h(rig, lambda n, K, Hm: Hm)),
            ("shift 60", with_h(rig, lambda n, K, Hm: shift(60, 0) @ Hm)),
            ("yaw 15", with_h(rig, lambda n, K, Hm: rotated(oracle, K, Hm, cfg, "y", 15.0))),
            ("zoom 0.5", with_h(rig, lambda n, K, Hm: C @ np.diag([0.5, 0.5, 1.0]) @ Hm)),
            ("singular", with_h(rig, lambda n, K, Hm: singular(Hm))),
            ("front alone", with_h(rig, lambda n, K, Hm: rotated(oracle, K, Hm, cfg, "x", -2.0) if n == "front" else Hm))]


def mixed_rigs(oracle, rig, cfg=CFG):
    """the table of the mode cases: the four smooth families and the rig's own H, five frame sets"""
    return smooth_rigs(oracle, rig, cfg) + [("own H", rig)]


def table(rigs):
    """[(name, rig)] -> float64 [B, 4, 3, 3]"""
    return np.ascontiguousarray(np.stack([np.stack([np.asarray(r[n][2], np.float64).reshape(3, 3) for n in CAMERAS]) for _, r in rigs]))


def frames_for(rng, batch, cfg=CFG):
    """random frame sets [batch, 4, FH, FW, 3], the back camera at half brightness"""
    f = rng.integers(0, 256, (batch, 4, cfg["FRAME_HEIGHT"], cfg["FRAME_WIDTH"], 3), dtype=np.uint8)
    f[:, 1] //= 2
    return f


# ---------------------------------------------------------------------------------------------------------------
# yardstick A: the oracle of the rig with H_b, per frame set; yardstick B: a fresh generator of the existing library
# ---------------------------------------------------------------------------------------------------------------
def oracle_images(oracle, rigs, frames, car, blend, cfg=CFG):
    """-> (images [B, BH, BW, 3], the pixels no camera covers)"""
    refs = [oracle.RefBevGenerator(r, cfg, blend=blend) for _, r in rigs]
    return np.stack([ref(*frames[b], car) for b, ref in enumerate(refs)]), H.uncovered(refs[0])


def library_images(SB, rigs, frames, car, blend, cfg=CFG, **kw):
    """frame set b through BevGenerator(rig=rig_b).batch: the static path of the library as it was"""
    return np.stack([H.generator(SB, r, cfg, blend=blend, **kw).batch(frames[b:b + 1], car)[0] for b, (_, r) in enumerate(rigs)])


def assert_images(got, want, none, what):
    """[B, BH, BW, 3] at tolerance 0, the pixels no camera covers first"""
    assert got.shape == want.shape and got.dtype == np.uint8, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    for b in range(got.shape[0]):
        H.assert_same(got[b], want[b], none, "%s, frame set %d" % (what, b))


# ---------------------------------------------------------------------------------------------------------------
# the census on the oracle
# ---------------------------------------------------------------------------------------------------------------
def lut_change(ref_static, ref_moving):
    """per camera, the share of masked BEV-table entries (texel or fraction) that differ between two oracles"""
    out = []
    for a, b, m in zip(ref_static.cameras, ref_moving.cameras, ref_static.masks):
        on = np.asarray(m) != 0
        diff = np.any(a.bev_maps[0] != b.bev_maps[0], axis=-1) | (a.bev_maps[1] != b.bev_maps[1])
        out.append(float(diff[on].mean()))
    return out


def grid_position(oracle, cam, cfg=CFG):
    """the integer undistorted-grid position (top-left texel) of every BEV pixel of an oracle camera"""
    xy, _ = oracle.perspective_coords(oracle.invert3x3(cam.H), (cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]))
    return xy.astype(np.int32)


def grid_census(oracle, ref, cfg=CFG):
    """per camera: (share of masked pixels whose 2 x 2 footprint lies wholly outside the undistorted grid, number of masked pixels whose
    footprint straddles the grid's edge)"""
    uw, uh = int(cfg["FRAME_WIDTH"] * cfg["SIZE_SCALE"]), int(cfg["FRAME_HEIGHT"] * cfg["SIZE_SCALE"])
    out = []
    for cam, m in zip(ref.cameras, ref.masks):
        on = np.asarray(m) != 0
        xy = grid_position(oracle, cam, cfg)
        outside = H.outside_of(xy, uw, uh)
        inside = (xy[..., 0] >= 0) & (xy[..., 0] < uw - 1) & (xy[..., 1] >= 0) & (xy[..., 1] < uh - 1)
        out.append((float(outside[on].mean()), int((~outside & ~inside & on).sum())))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------------------------------------------
def run_step(ffi, bev, frames, hs, car, off_frames=0, off_out=0, off_car=0, poison=True, guard=256):
    """One step on buffers of exactly the batch's bytes between FILL guards (off_*: byte offsets that misalign a buffer).  hs: float64
    [B, 4, 3, 3] -> bevw_run_homographies_device, the caller's array overwritten with NaN as soon as the call returns and before the sync
    (poison); None -> bevw_run_device.  -> (images [B, BH, pitch, 3] with the padding columns, the path of the step).  A refused step
    raises after the guards AND the batch's bytes were found untouched."""
    B = frames.shape[0]
    c = bev._engine.cfg
    need = B * bev.out_image_bytes
    d_in = ffi.DeviceBuffer(frames.nbytes + 8)
    d_out = ffi.DeviceBuffer(guard + need + guard + 8)
    d_car = ffi.DeviceBuffer(car.nbytes + 8) if car is not None else None
    try:
        d_in.upload(frames, off_frames)
        if d_car:
            d_car.upload(car, off_car)
        d_out.fill(FILL)
        args = (d_car.ptr + off_car if d_car else None, d_out.ptr + guard + off_out)
        try:
            if hs is None:
                bev.run_device(d_in.ptr + off_frames, B, *args, out_bytes=need)
            else:
                hs = np.array(hs, np.float64)   # a copy the step may poison
                bev.run_homographies_device(d_in.ptr + off_frames, hs, B, *args, out_bytes=need)
                if poison:
                    hs[...] = np.nan
        except Exception:
            bev.sync()
            assert (d_out.download((d_out.nbytes,)) == FILL).all(), "a refused step wrote to the output buffer"
            raise
        bev.sync()
        raw = d_out.download((guard + need + guard + 8,))
        before, after = raw[:guard + off_out], raw[guard + off_out + need:]
        assert (before == FILL).all() and (after == FILL).all(), "bytes outside the batch's %d were written" % need
        return raw[guard + off_out:guard + off_out + need].reshape(B, c.bev_height, bev.out_pitch, 3).copy(), bev.last_path()
    finally:
        d_in.free()
        d_out.free()
        if d_car:
            d_car.free()
