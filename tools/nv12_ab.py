#!/usr/bin/env python3
"""A/B of the NV12 input path (bevw_set_input_format) against the BGR one, in ONE process.

For each workload a BGR and an NV12 handle are built on the same rig and fed the same seeded frames: `--unique` random NV12 frame sets,
and for the BGR handle their conversion by the NumPy specification (tests/_nv12_spec.py, i.e. cv2.cvtColor(COLOR_YUV2BGR_NV12)),
replicated over the batch in device memory.  After a warm-up the two handles alternate (order swapped every round) over `--rounds`
rounds of `--steps` timed steps on device-resident buffers; every step is bracketed by the handle's timer marks, and the median ms per
step of each handle is reported with its ratio.  Both handles must also return the same bytes (checked on two frame sets).

    python tools/nv12_ab.py [--workloads config3,config4,undistort] [--rounds 5] [--steps 20] [--warmup 10]

Workloads: config3 = BASELINE config 3 (1280 x 960 -> 1080 x 1080, direct, batch 256, pitched device images), config4 = blend + balance
on the same rig (batch 256, pitched), undistort = BASELINE config 2 geometry (fisheye remap, batch 64).  One JSON line per workload, then
a summary line; the bar of the NV12 feature is config3 nv12 / bgr <= 1.2.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/nv12_ab.py ...` (a run of its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cameracalibration_amd import _ffi, workloads as W  # noqa: E402
from tests import _nv12_spec as S  # noqa: E402

# Algorithmic bytes per frame set (workloads.ALGORITHMIC_BYTES) and their NV12 counterparts: the source bytes a step must read at 1.5 bytes
# per touched texel instead of 3 (the chroma of 2 x 2 blocks that are touched only in part is not counted), the output bytes unchanged.
ALG = {
    "config3": ("direct_stitch_b256", 5_532_357, 2_033_157 // 2 + 3_499_200),
    "config4": ("blend_balance_b256", 22_585_476, 14_745_600 // 2 + 2_170_338 + 3_499_200),
    "undistort": ("undistort_b64", 5_421_912, 1_735_512 // 2 + 3_686_400),
}


def replicated(unique: np.ndarray, batch: int, device: int = 0) -> "_ffi.DeviceBuffer":
    buf = _ffi.DeviceBuffer(batch * unique[0].nbytes, device)
    for b in range(batch):
        buf.upload(unique[b % len(unique)], b * unique[0].nbytes)
    return buf


class Stitch:
    def __init__(self, fmt, unique, batch, blend, balance):
        from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

        ns = SB.BevGenerator.get_args()
        for k, v in W.CONFIG_S.items():
            setattr(ns, k, v)
        self.g = SB.BevGenerator(blend=blend, balance=balance, rig=W.rig_s(), output_pitch="auto", input_format=fmt)
        self.batch = batch
        self.d_in = replicated(unique, batch)
        self.d_out = _ffi.DeviceBuffer(batch * self.g.out_image_bytes)
        self.sync, self.tstart, self.tstop = self.g.sync, self.g.timer_start, self.g.timer_stop
        self.tmark, self.tbetween = self.g.timer_mark, self.g.timer_between

    def step(self):
        self.g.run_device(self.d_in.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        c = W.CONFIG_S
        return self.d_out.download((c["BEV_HEIGHT"], self.g.out_pitch, 3), offset=b * self.g.out_image_bytes)[:, :c["BEV_WIDTH"]]


class Remap:
    def __init__(self, fmt, unique, batch, channels=3):
        """channels=1: a one-channel remapper on frames [height, width] (tools/gray_ab.py)."""
        from cameracalibration_amd.Tools import undistort as U

        c = W.CONFIG_UNDISTORT
        K, D = W.undistort_calibration()
        self.u = U.Undistorter(K, D, c["FRAME_WIDTH"], c["FRAME_HEIGHT"], focalscale=c["FOCAL_SCALE"], sizescale=c["SIZE_SCALE"],
                               input_format=fmt, channels=channels)
        self.batch, self.r, L = batch, self.u._r, _ffi.lib()
        self.d_in = replicated(unique, batch)
        self.img = self.u.out_image_bytes
        self.d_out = _ffi.DeviceBuffer(batch * self.img)
        self.sync = lambda: _ffi.check(L.bevw_remapper_sync(self.r))
        self.tstart = lambda: _ffi.check(L.bevw_remapper_timer_start(self.r))
        self.tmark = lambda i: _ffi.check(L.bevw_remapper_timer_mark(self.r, i))

        def tstop():
            ms = C.c_float()
            _ffi.check(L.bevw_remapper_timer_stop(self.r, C.byref(ms)))
            return float(ms.value)

        def tbetween(a, b):
            ms = C.c_float()
            _ffi.check(L.bevw_remapper_timer_between(self.r, a, b, C.byref(ms)))
            return float(ms.value)
        self.tstop, self.tbetween = tstop, tbetween

    def step(self):
        _ffi.check(_ffi.lib().bevw_remap_device(self.r, self.d_in.ptr, self.batch, self.d_out.ptr))

    def fetch(self, b):
        return self.d_out.download((self.u.out_h, self.u.out_w) + ((3,) if self.u.channels == 3 else ()), offset=b * self.img)


def timed(run, steps):
    run.tstart()
    for i in range(steps):
        run.tmark(i)
        run.step()
    run.tmark(steps)
    run.tstop()
    return [run.tbetween(i, i + 1) for i in range(steps)]


def ab(name, runs, a):
    for r in runs.values():
        for _ in range(a.warmup):
            r.step()
        r.sync()
    laps = {k: [] for k in runs}
    rounds = {k: [] for k in runs}
    names = list(runs)
    for k in range(a.rounds):
        for fmt in (names if k % 2 == 0 else names[::-1]):
            t = timed(runs[fmt], a.steps)
            laps[fmt] += t
            rounds[fmt].append(statistics.median(t))
    same = all(np.array_equal(runs["bgr"].fetch(b), runs["nv12"].fetch(b)) for b in (0, min(17, runs["bgr"].batch - 1)))
    med = {k: statistics.median(v) for k, v in laps.items()}
    key, alg_bgr, alg_nv12 = ALG[name]
    return {"workload": name, "baseline_workload": key, "batch": runs["bgr"].batch, "rounds": a.rounds, "steps_per_round": a.steps,
            "ms_per_step": {k: round(v, 5) for k, v in med.items()}, "round_medians_ms": {k: [round(x, 5) for x in v] for k, v in rounds.items()},
            "nv12_over_bgr": round(med["nv12"] / med["bgr"], 4), "outputs_identical": bool(same),
            "algorithmic_bytes_per_set": {"bgr": alg_bgr, "nv12": alg_nv12},
            "algorithmic_gbs": {k: round(b * runs[k].batch / (med[k] * 1e-3) / 1e9, 1) for k, b in (("bgr", alg_bgr), ("nv12", alg_nv12))}}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workloads", default="config3,config4,undistort")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--unique", type=int, default=16, help="distinct frame sets, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    a = p.parse_args()
    _ffi.require_device()
    rng = np.random.default_rng(a.seed)
    out = []
    for name in a.workloads.split(","):
        if name in ("config3", "config4"):
            c = W.CONFIG_S
            nv = S.random_nv12(rng, (a.unique, 4), c["FRAME_WIDTH"], c["FRAME_HEIGHT"])
            bgr = S.nv12_to_bgr(nv)
            blend = balance = name == "config4"
            runs = {"bgr": Stitch("bgr", bgr, 256, blend, balance), "nv12": Stitch("nv12", nv, 256, blend, balance)}
        elif name == "undistort":
            c = W.CONFIG_UNDISTORT
            nv = S.random_nv12(rng, (a.unique,), c["FRAME_WIDTH"], c["FRAME_HEIGHT"])
            runs = {"bgr": Remap("bgr", S.nv12_to_bgr(nv), 64), "nv12": Remap("nv12", nv, 64)}
        else:
            raise SystemExit("unknown workload %s" % name)
        r = ab(name, runs, a)
        print(json.dumps(r), flush=True)
        out.append(r)
        for run in runs.values():
            run.d_in.free()
            run.d_out.free()
    c3 = [r for r in out if r["workload"] == "config3"]
    print(json.dumps({"summary": {r["workload"]: r["nv12_over_bgr"] for r in out},
                      "config3_bar_1_2": (c3[0]["nv12_over_bgr"] <= 1.2) if c3 else None,
                      "all_outputs_identical": all(r["outputs_identical"] for r in out)}), flush=True)


if __name__ == "__main__":
    main()
