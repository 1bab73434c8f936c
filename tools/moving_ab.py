#!/usr/bin/env python3
"""A/B of the stitch with a homography per frame set (bevw_run_homographies_device) against the static steps and against what a caller
with moving extrinsics does without it, in ONE process.

At the geometry of workloads.CONFIG_S (4 x 1280 x 960 -> 1080 x 1080), direct and blend, batches 64 and 256, on device-resident buffers:
  (M)   the new step, every frame set with a random pitch within +-2 degrees (all four cameras), aligned output pitch;
  (M0)  the new step with every matrix equal to the handle's own, same handle;
  (M0d) (M0) on the dense per-pixel handle of (P): the like-for-like partner of (P);
  (P)   bevw_run_device on the per-pixel schedule (dense rows);
  (U)   bevw_run_device on the units (aligned output pitch);
  (R)   what a caller does today: per frame set four bevw_set_camera + bevw_build + a batch-1 bevw_run_device on one handle, then one
        sync, timed wall-clock over `--rebuild-sets` frame sets -- with the library given by --parent-lib (the parent commit's build:
        BEVW_BUILD_TAG=parent python -m cameracalibration_amd.build), loaded beside the current one.
Before any timing (M0)'s images are compared with (U)'s and (M0d)'s with (P)'s, byte for byte, and the paths are read (bevw_last_path).
After a warm-up of every shape the device variants alternate (order reversed every round) over `--rounds` rounds of `--steps` timed steps,
every step bracketed by the handle's timer marks (device events); medians of the per-step times are reported.

    python tools/moving_ab.py --parent-lib build_var/libbevwarp_parent.so [--batches 64,256] [--modes direct,blend] [--out FILE]

One JSON line per (mode, batch) and a table at the end (also written to --out).  The one bar: (M) per frame set < (R) per frame set in
every row.  M0 / P and M / U are reported, not barred."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nv12_ab as AB  # noqa: E402  (replicated, timed)
from cameracalibration_amd import _ffi, workloads as W  # noqa: E402

CAMERAS = ("front", "back", "left", "right")


def pitched(K, Hm, cfg, degrees):
    """H of a camera pitched by `degrees`: H @ inv(Kd R Kd^-1), Kd the camera matrix of the undistorted grid (camera_mat_dst)"""
    Kd = np.array(K, np.float64)
    Kd[0, 0] *= cfg["FOCAL_SCALE"]
    Kd[1, 1] *= cfg["FOCAL_SCALE"]
    Kd[0, 2] = cfg["FRAME_WIDTH"] / 2 * cfg["SIZE_SCALE"]
    Kd[1, 2] = cfg["FRAME_HEIGHT"] / 2 * cfg["SIZE_SCALE"]
    a = np.deg2rad(degrees)
    R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return Hm @ np.linalg.inv(Kd @ R @ np.linalg.inv(Kd))


class Step:
    """One generator over the shared device-resident frames; hs: the table of a moving step, None: bevw_run_device."""

    def __init__(self, gen, d_in, batch, hs):
        self.g, self.d_in, self.batch, self.hs = gen, d_in, batch, hs
        self.d_out = _ffi.DeviceBuffer(batch * gen.out_image_bytes)
        self.sync, self.tstart, self.tstop, self.tmark, self.tbetween = gen.sync, gen.timer_start, gen.timer_stop, gen.timer_mark, gen.timer_between

    def step(self):
        if self.hs is None:
            self.g.run_device(self.d_in.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)
        else:
            self.g.run_homographies_device(self.d_in.ptr, self.hs, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        c = W.CONFIG_S
        return self.d_out.download((c["BEV_HEIGHT"], self.g.out_pitch, 3), offset=b * self.g.out_image_bytes)[:, :c["BEV_WIDTH"]]


def generator(blend, **kw):
    from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

    ns = SB.BevGenerator.get_args()
    for k, v in W.CONFIG_S.items():
        setattr(ns, k, v)
    return SB.BevGenerator(blend=blend, balance=False, rig=W.rig_s(), **kw)


def rebuild_per_frame_set(path, blend, tables, d_in, set_bytes, sets):
    """(R): ms per frame set, wall clock, with the library at `path`"""
    L = C.CDLL(path)
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    c, rig = W.CONFIG_S, W.rig_s()
    cfg = _ffi.bevw_config(c["FRAME_WIDTH"], c["FRAME_HEIGHT"], c["BEV_WIDTH"], c["BEV_HEIGHT"], c["CAR_WIDTH"], c["CAR_HEIGHT"], c["FOCAL_SCALE"],
                           c["SIZE_SCALE"], int(blend), 0, 0, _ffi.SCHED_AUTO)
    h = C.c_void_p()

    def ok(s):
        assert s == 0, L.bevw_last_error()

    ok(L.bevw_create(C.byref(cfg), C.byref(h)))
    img = c["BEV_WIDTH"] * c["BEV_HEIGHT"] * 3
    d_out = _ffi.DeviceBuffer(sets * img)
    KD = [(_ffi.f64(rig[n][0], 9), _ffi.f64(rig[n][1], 4)) for n in CAMERAS]

    def one(b):
        for i in range(4):
            ok(L.bevw_set_camera(h, i, _ffi.ptr(KD[i][0]), _ffi.ptr(KD[i][1]), _ffi.ptr(np.ascontiguousarray(tables[b, i]))))
        ok(L.bevw_build(h))
        ok(L.bevw_run_device(h, d_in.ptr + b * set_bytes, 1, None, d_out.ptr + b * img))

    try:
        one(0)                       # warm-up: code objects, first allocations
        ok(L.bevw_sync(h))
        t0 = time.perf_counter()
        for b in range(sets):
            one(b)
        ok(L.bevw_sync(h))
        ms = (time.perf_counter() - t0) * 1e3 / sets
        last = d_out.download((c["BEV_HEIGHT"], c["BEV_WIDTH"], 3), offset=(sets - 1) * img)
    finally:
        L.bevw_destroy(h)
        d_out.free()
    return ms, last


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--parent-lib", required=True, help="libbevwarp.so of the parent commit, for (R)")
    p.add_argument("--batches", default="64,256")
    p.add_argument("--modes", default="direct,blend")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rebuild-sets", type=int, default=16)
    p.add_argument("--unique", type=int, default=8, help="distinct frame sets, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert os.path.exists(a.parent_lib), a.parent_lib
    _ffi.require_device()
    c, rig = W.CONFIG_S, W.rig_s()
    batches = [int(b) for b in a.batches.split(",")]
    rng = np.random.default_rng(a.seed)
    frames = rng.integers(0, 256, (a.unique, 4, c["FRAME_HEIGHT"], c["FRAME_WIDTH"], 3), dtype=np.uint8)
    d_in = AB.replicated(frames, max(batches))
    set_bytes = frames[0].nbytes
    own = np.stack([rig[n][2] for n in CAMERAS])
    moving = np.stack([np.stack([pitched(rig[n][0], rig[n][2], c, deg) for n in CAMERAS]) for deg in rng.uniform(-2.0, 2.0, max(batches))])
    rows = []
    for mode in a.modes.split(","):
        blend = {"direct": False, "blend": True}[mode]
        r_ms, r_last = rebuild_per_frame_set(a.parent_lib, blend, moving, d_in, set_bytes, a.rebuild_sets)
        for batch in batches:
            units, pp = generator(blend, output_pitch="aligned"), generator(blend, output_pitch="dense", schedule=_ffi.SCHED_PER_PIXEL)
            own_b = np.ascontiguousarray(np.broadcast_to(own, (batch, 4, 3, 3)))
            runs = {"M": Step(units, d_in, batch, np.ascontiguousarray(moving[:batch])), "M0": Step(units, d_in, batch, own_b),
                    "M0d": Step(pp, d_in, batch, own_b), "P": Step(pp, d_in, batch, None), "U": Step(units, d_in, batch, None)}
            paths = {}
            for k, r in runs.items():
                for _ in range(a.warmup):
                    r.step()
                r.sync()
                paths[k] = r.g.last_path()
            probe = (0, min(17, batch - 1), batch - 1)
            same = {"M0_is_U": all(np.array_equal(runs["M0"].fetch(b), runs["U"].fetch(b)) for b in probe),
                    "M0d_is_P": all(np.array_equal(runs["M0d"].fetch(b), runs["P"].fetch(b)) for b in probe),
                    "M_is_R": bool(np.array_equal(runs["M"].fetch(a.rebuild_sets - 1), r_last)) if batch >= a.rebuild_sets else None}
            laps, names = {k: [] for k in runs}, list(runs)
            for k in range(a.rounds):
                for name in (names if k % 2 == 0 else names[::-1]):
                    laps[name] += AB.timed(runs[name], a.steps)
            med = {k: statistics.median(v) for k, v in laps.items()}
            row = {"mode": mode, "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps, "paths": paths, "ms_per_step": {k: round(v, 4) for k, v in med.items()},
                   "M_us_per_frame_set": round(med["M"] * 1e3 / batch, 2), "R_us_per_frame_set": round(r_ms * 1e3, 1), "R_over_M": round(r_ms * batch / med["M"], 1),
                   "M0_over_U": round(med["M0"] / med["U"], 3), "M0d_over_P": round(med["M0d"] / med["P"], 3), "M_over_U": round(med["M"] / med["U"], 3),
                   "M_over_M0": round(med["M"] / med["M0"], 3), "bar_M_lt_R": bool(med["M"] / batch < r_ms), **same}
            print(json.dumps(row), flush=True)
            rows.append(row)
            for r in runs.values():
                r.d_out.free()
            units._engine.close()
            pp._engine.close()
    d_in.free()
    lines = ["mode    batch |   M ms   M0 ms  M0d ms    P ms    U ms | M us/set   R us/set   R/M | M0/U  M0d/P  M/U   M/M0"]
    for r in rows:
        m = r["ms_per_step"]
        lines.append("%-7s %5d | %6.3f  %6.3f  %6.3f  %6.3f  %6.3f | %8.2f  %9.1f  %5.0f | %5.2f  %5.2f  %5.2f  %5.2f" % (
            r["mode"], r["batch"], m["M"], m["M0"], m["M0d"], m["P"], m["U"], r["M_us_per_frame_set"], r["R_us_per_frame_set"], r["R_over_M"], r["M0_over_U"],
            r["M0d_over_P"], r["M_over_U"], r["M_over_M0"]))
    ok = {"bar_M_lt_R_in_every_row": all(r["bar_M_lt_R"] for r in rows), "M0_is_U": all(r["M0_is_U"] for r in rows), "M0d_is_P": all(r["M0d_is_P"] for r in rows),
          "M_is_R": all(r["M_is_R"] for r in rows if r["M_is_R"] is not None)}
    lines.append(json.dumps(ok))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")
    assert all(ok.values()), ok


if __name__ == "__main__":
    main()
