#!/usr/bin/env python3
"""A/B of the one-channel stitch (bevw_set_channels: BevGenerator(channels=1)) against the three-channel one, in ONE process.

At the geometry of workloads.CONFIG_S (BASELINE config 3: 4 x 1280 x 960 -> 1080 x 1080, aligned output pitch), direct and blend, batches
64 and 256, on device-resident buffers, three generators of the same rig:
  (a) gray            the one-channel step on `--unique` seeded random grey frame sets (replicated over the batch);
  (b) bgr             the three-channel step of the same geometry on random BGR frame sets (the kernels every BGR caller runs);
  (c) bgr_replicated  what a grey-camera caller does today: the three-channel step on the grey frames replicated to B = G = R (the
                      replicate and extract passes are not even counted);
  (d) gray_parent     with --parent-lib: (a)'s step of ANOTHER build of the library -- the parent commit's -- loaded beside this one, on
                      (a)'s frames; its images are compared with (a)'s, and (a) <= (d) x (1 + the relative spread of (d) over the rounds).
Before any timing (a)'s images are compared with channel 0 of (c)'s and the path of every generator is read (bevw_last_path).  After a
warm-up of every shape the variants alternate (order reversed every round) over `--rounds` rounds of `--steps` timed steps; every step is
bracketed by the handle's timer marks, and the median ms per step is reported.

    python tools/gray_stitch_ab.py [--parent-lib <libbevwarp.so of the parent commit>] [--batches 64,256] [--modes direct,blend] [--rounds 5] [--steps 20] [--warmup 10]

One JSON line per (mode, batch): ms per step, (a) / (b), and (a)'s bytes (frames + images, from the shapes) over its time beside the copy
yardstick (bevw_device_copy_rate).  The bar: the grey step moves a third of the bytes through the same partition with the same number of
requests, so (a) <= (b) in every row."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nv12_ab as AB  # noqa: E402  (replicated, timed)
from cameracalibration_amd import _ffi, workloads as W  # noqa: E402


def load(path):
    """Another build of the library beside the bound one: the signatures it has (tools/nearest_ab.py)."""
    L = C.CDLL(path)
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


class Stitch:
    """One generator over device-resident inputs shared between the modes; d_in holds at least `batch` frame sets."""

    def __init__(self, channels, blend, d_in, batch):
        from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

        ns = SB.BevGenerator.get_args()
        for k, v in W.CONFIG_S.items():
            setattr(ns, k, v)
        self.g = SB.BevGenerator(blend=blend, balance=False, rig=W.rig_s(), output_pitch="aligned", channels=channels)
        self.channels, self.batch, self.d_in = channels, batch, d_in
        self.d_out = _ffi.DeviceBuffer(batch * self.g.out_image_bytes)
        self.sync, self.tstart, self.tstop = self.g.sync, self.g.timer_start, self.g.timer_stop
        self.tmark, self.tbetween, self.last_path = self.g.timer_mark, self.g.timer_between, self.g.last_path

    def step(self):
        self.g.run_device(self.d_in.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        c = W.CONFIG_S
        shape = (c["BEV_HEIGHT"], self.g.out_pitch) + ((3,) if self.channels == 3 else ())
        return self.d_out.download(shape, offset=b * self.g.out_image_bytes)[:, :c["BEV_WIDTH"]]

    def close(self):
        self.d_out.free()
        self.g._engine.close()


class LibStitch:
    """Stitch(1, ...) on the C entry points of library L (another build, loaded beside the bound one): the same configuration, rig, aligned
    output pitch and one channel, as BevGenerator sets them; the device buffers are the process's, whichever build runs on them."""

    def __init__(self, L, blend, d_in, batch):
        c = W.CONFIG_S
        self.L, self.batch, self.d_in, self.h = L, batch, d_in, C.c_void_p()
        cfg = _ffi.bevw_config(c["FRAME_WIDTH"], c["FRAME_HEIGHT"], c["BEV_WIDTH"], c["BEV_HEIGHT"], c["CAR_WIDTH"], c["CAR_HEIGHT"],
                               float(c["FOCAL_SCALE"]), float(c["SIZE_SCALE"]), int(blend), 0, 0, _ffi.SCHED_AUTO)
        self.check(L.bevw_create(C.byref(cfg), C.byref(self.h)))
        rig = W.rig_s()
        for i, n in enumerate(W.CAMERA_NAMES):
            K, D, H = rig[n]
            self.check(L.bevw_set_camera(self.h, i, _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(D, 4)), _ffi.ptr(_ffi.f64(H, 9))))
        self.check(L.bevw_set_output_pitch(self.h, _ffi.PITCH_ALIGNED))
        self.check(L.bevw_set_channels(self.h, 1))
        self.check(L.bevw_build(self.h))
        self.out_pitch = int(L.bevw_output_pitch(self.h))
        self.out_image_bytes = self.out_pitch * c["BEV_HEIGHT"]
        self.d_out = _ffi.DeviceBuffer(batch * self.out_image_bytes)

    def check(self, status):
        if status != 0:
            raise RuntimeError(self.L.bevw_last_error().decode("utf-8", "replace"))

    def step(self):
        self.check(self.L.bevw_run_device(self.h, self.d_in.ptr, self.batch, None, self.d_out.ptr))

    def sync(self):
        self.check(self.L.bevw_sync(self.h))

    def tstart(self):
        self.check(self.L.bevw_timer_start(self.h))

    def tstop(self):
        ms = C.c_float()
        self.check(self.L.bevw_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def tmark(self, slot):
        self.check(self.L.bevw_timer_mark(self.h, int(slot)))

    def tbetween(self, a, b):
        ms = C.c_float()
        self.check(self.L.bevw_timer_between(self.h, int(a), int(b), C.byref(ms)))
        return ms.value

    def last_path(self):
        return int(self.L.bevw_last_path(self.h))

    def fetch(self, b):
        c = W.CONFIG_S
        return self.d_out.download((c["BEV_HEIGHT"], self.out_pitch), offset=b * self.out_image_bytes)[:, :c["BEV_WIDTH"]]

    def close(self):
        self.d_out.free()
        self.L.bevw_destroy(self.h)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batches", default="64,256")
    p.add_argument("--modes", default="direct,blend")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--unique", type=int, default=8, help="distinct frame sets, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--parent-lib", default=None, help="libbevwarp.so built from the parent commit: its one-channel step is timed as gray_parent")
    a = p.parse_args()
    _ffi.require_device()
    P = load(a.parent_lib) if a.parent_lib else None
    copy_gbs = _ffi.device_copy_rate()
    print(json.dumps({"copy_kernel_gbs_moved": round(copy_gbs, 1)}), flush=True)
    c = W.CONFIG_S
    fw, fh, bw, bh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"], c["BEV_WIDTH"], c["BEV_HEIGHT"]
    batches = [int(b) for b in a.batches.split(",")]
    rng = np.random.default_rng(a.seed)
    gray = rng.integers(0, 256, (a.unique, 4, fh, fw), dtype=np.uint8)
    bgr = rng.integers(0, 256, (a.unique, 4, fh, fw, 3), dtype=np.uint8)
    inputs = {"gray": AB.replicated(gray, max(batches)), "bgr": AB.replicated(bgr, max(batches)),
              "bgr_replicated": AB.replicated(np.ascontiguousarray(gray[..., None].repeat(3, -1)), max(batches))}
    out = []
    for mode in a.modes.split(","):
        blend = {"direct": False, "blend": True}[mode]
        for batch in batches:
            runs = {k: Stitch(1 if k == "gray" else 3, blend, d, batch) for k, d in inputs.items()}
            if P is not None:
                runs["gray_parent"] = LibStitch(P, blend, inputs["gray"], batch)
            for r in runs.values():
                for _ in range(a.warmup):
                    r.step()
                r.sync()
            paths = {k: r.last_path() for k, r in runs.items()}
            same = all(np.array_equal(runs["gray"].fetch(b), runs["bgr_replicated"].fetch(b)[..., 0]) for b in (0, min(17, batch - 1), batch - 1))
            laps, names = {k: [] for k in runs}, list(runs)
            for k in range(a.rounds):
                for name in (names if k % 2 == 0 else names[::-1]):
                    laps[name] += AB.timed(runs[name], a.steps)
            med = {k: statistics.median(v) for k, v in laps.items()}
            gray_bytes = batch * (4 * fw * fh + runs["gray"].g.out_image_bytes)
            r = {"workload": "config3", "mode": mode, "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps, "paths": paths,
                 "out_pitch": runs["gray"].g.out_pitch, "ms_per_step": {k: round(v, 5) for k, v in med.items()},
                 "gray_over_bgr": round(med["gray"] / med["bgr"], 4), "gray_over_bgr_replicated": round(med["gray"] / med["bgr_replicated"], 4),
                 "gray_not_slower_than_bgr": bool(med["gray"] <= med["bgr"]), "gray_bytes_frames_plus_images": gray_bytes,
                 "gray_gbs": round(gray_bytes / (med["gray"] * 1e-3) / 1e9, 1), "copy_kernel_gbs_moved": round(copy_gbs, 1), "outputs_identical": bool(same)}
            if P is not None:
                # the rounds' medians of the two builds' one-channel steps, the parent's relative spread over them, and the bar it sets
                rounds = {k: [statistics.median(laps[k][i * a.steps:(i + 1) * a.steps]) for i in range(a.rounds)] for k in ("gray", "gray_parent")}
                spread = (max(rounds["gray_parent"]) - min(rounds["gray_parent"])) / med["gray_parent"]
                same = same and all(np.array_equal(runs["gray"].fetch(b), runs["gray_parent"].fetch(b)) for b in (0, min(17, batch - 1), batch - 1))
                r.update({"rounds_ms": {k: [round(x, 5) for x in v] for k, v in rounds.items()}, "gray_over_gray_parent": round(med["gray"] / med["gray_parent"], 4),
                          "gray_parent_relative_spread": round(spread, 4), "gray_not_slower_than_parent": bool(med["gray"] <= med["gray_parent"] * (1.0 + spread)),
                          "outputs_identical": bool(same)})
            print(json.dumps(r), flush=True)
            out.append(r)
            for run in runs.values():
                run.close()
    for d in inputs.values():
        d.free()
    ok = {"bar_gray_le_bgr": all(r["gray_not_slower_than_bgr"] for r in out),
          "all_units": all(set(r["paths"].values()) == {_ffi.PATH_UNITS} for r in out), "all_outputs_identical": all(r["outputs_identical"] for r in out)}
    print(json.dumps({"summary": {"%s_b%d" % (r["mode"], r["batch"]): r["gray_over_bgr"] for r in out}, **ok}), flush=True)
    assert ok["all_units"] and ok["all_outputs_identical"], ok


if __name__ == "__main__":
    main()
