#!/usr/bin/env python3
"""A/B of the one-channel remapper (bevw_remapper_set_channels: Undistorter(channels=1)) against the three-channel one, in ONE process.

At the geometry of workloads.CONFIG_UNDISTORT and batches 64 and 256, on device-resident buffers, three remappers over the same maps:
  (a) gray            the one-channel step on `--unique` seeded random grey frames (replicated over the batch);
  (b) bgr             the three-channel step of the same geometry on random BGR frames;
  (c) bgr_replicated  what a caller without the mode does today: the three-channel step on the grey frames replicated to B = G = R (the
                      replicate and extract passes are not even counted).
Before any timing (a)'s images are compared with channel 0 of (c)'s and the path of every remapper is read (bevw_remapper_last_path).
After a warm-up of every shape the variants alternate (order reversed every round) over `--rounds` rounds of `--steps` timed steps; every
step is bracketed by the remapper's timer marks, and the median ms per step is reported.

    python tools/gray_ab.py [--batches 64,256] [--rounds 5] [--steps 20] [--warmup 10]

One JSON line per batch: ms per step, (a) / (b), and (a)'s bytes (src + dst, from the shapes) over its time beside the copy yardstick
(bevw_device_copy_rate).  The bar: the grey step runs the same plan and entries on a third of the image bytes, so (a) <= (b) at both batches.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gray_ab.py ...` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nv12_ab as AB  # noqa: E402  (Remap, replicated, timed)
from cameracalibration_amd import _ffi, workloads as W  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batches", default="64,256")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--unique", type=int, default=16, help="distinct frames, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    a = p.parse_args()
    _ffi.require_device()
    copy_gbs = _ffi.device_copy_rate()
    print(json.dumps({"copy_kernel_gbs_moved": round(copy_gbs, 1)}), flush=True)
    c = W.CONFIG_UNDISTORT
    fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
    rng = np.random.default_rng(a.seed)
    gray = rng.integers(0, 256, (a.unique, fh, fw), dtype=np.uint8)
    bgr = rng.integers(0, 256, (a.unique, fh, fw, 3), dtype=np.uint8)
    L = _ffi.lib()
    out = []
    for batch in (int(b) for b in a.batches.split(",")):
        runs = {"gray": AB.Remap("bgr", gray, batch, channels=1), "bgr": AB.Remap("bgr", bgr, batch),
                "bgr_replicated": AB.Remap("bgr", np.ascontiguousarray(gray[..., None].repeat(3, -1)), batch)}
        for r in runs.values():
            for _ in range(a.warmup):
                r.step()
            r.sync()
        paths = {k: int(L.bevw_remapper_last_path(r.r)) for k, r in runs.items()}
        same = all(np.array_equal(runs["gray"].fetch(b), runs["bgr_replicated"].fetch(b)[..., 0]) for b in (0, min(17, batch - 1)))
        laps, names = {k: [] for k in runs}, list(runs)
        for k in range(a.rounds):
            for name in (names if k % 2 == 0 else names[::-1]):
                laps[name] += AB.timed(runs[name], a.steps)
        med = {k: statistics.median(v) for k, v in laps.items()}
        u = runs["gray"].u
        gray_bytes = batch * (fw * fh + u.out_w * u.out_h)
        r = {"workload": "undistort", "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps, "paths": paths,
             "ms_per_step": {k: round(v, 5) for k, v in med.items()}, "gray_over_bgr": round(med["gray"] / med["bgr"], 4),
             "gray_over_bgr_replicated": round(med["gray"] / med["bgr_replicated"], 4), "gray_not_slower_than_bgr": bool(med["gray"] <= med["bgr"]),
             "gray_bytes_src_plus_dst": gray_bytes, "gray_gbs": round(gray_bytes / (med["gray"] * 1e-3) / 1e9, 1),
             "copy_kernel_gbs_moved": round(copy_gbs, 1), "outputs_identical": bool(same)}
        print(json.dumps(r), flush=True)
        out.append(r)
        for run in runs.values():
            run.d_in.free()
            run.d_out.free()
            run.u.close()
    print(json.dumps({"summary": {str(r["batch"]): r["gray_over_bgr"] for r in out}, "bar_gray_le_bgr": all(r["gray_not_slower_than_bgr"] for r in out),
                      "all_units": all(set(r["paths"].values()) == {_ffi.PATH_UNITS} for r in out),
                      "all_outputs_identical": all(r["outputs_identical"] for r in out)}), flush=True)


if __name__ == "__main__":
    main()
