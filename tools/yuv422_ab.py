#!/usr/bin/env python3
"""A/B of the packed 4:2:2 input path (bevw_set_input_format: YUYV) against the BGR and the NV12 ones, in ONE process.

For each workload a BGR, an NV12 and a YUYV handle are built on the same rig.  The YUYV handle is fed `--unique` seeded random frame sets,
the BGR handle their conversion by the NumPy specification (tests/_yuv422_spec.py, i.e. cv2.cvtColor(COLOR_YUV2BGR_YUY2)), the NV12
handle random NV12 frames of the same size; all replicated over the batch in device memory.  Before any timing the YUYV handle's images
are compared with the BGR handle's (two frame sets; NV12 images against the specification of the output conversion).  After a warm-up
the handles alternate (order reversed every round) over `--rounds` rounds of `--steps` timed steps on device-resident buffers; every step
is bracketed by the handle's timer marks, and the median ms per step of each handle is reported.

    python tools/yuv422_ab.py [--workloads config3,config3_nv12out,config4,undistort] [--rounds 5] [--steps 20] [--warmup 10]

Workloads: config3 = BASELINE config 3 (1280 x 960 -> 1080 x 1080, direct, batch 256, pitched device images), config3_nv12out = the same
writing NV12 images, config4 = blend + balance on the same rig (batch 256), undistort = BASELINE config 2 geometry (fisheye remap, batch 64).
One JSON line per workload, then a summary line with the two yardsticks on config 3:
  (a) yuyv / nv12 -- expected <= 1.05;
  (b) yuyv < bgr + a conversion pass (2 bytes read and 3 written per texel of the batch's frames) at the library's own copy-kernel
      rate (bevw_device_copy_rate): what a user without the format pays today.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/yuv422_ab.py ...` (a run of its own)."""
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
from tests import _nv12_out_spec as SO  # noqa: E402
from tests import _nv12_spec as SN  # noqa: E402
from tests import _yuv422_spec as S  # noqa: E402

# Algorithmic bytes per frame set: the touched texels (677,719 per config-3 set) at 2 bytes each + the output bytes
ALG = {
    "config3": {"bgr": 5_532_357, "nv12": 2_033_157 // 2 + 3_499_200, "yuyv": 1_355_438 + 3_499_200},
    "config3_nv12out": {"bgr": 2_033_157 + 1_749_600, "nv12": 2_033_157 // 2 + 1_749_600, "yuyv": 1_355_438 + 1_749_600},
}


class Stitch:
    def __init__(self, fmt, unique, batch, blend, balance, out):
        from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

        ns = SB.BevGenerator.get_args()
        for k, v in W.CONFIG_S.items():
            setattr(ns, k, v)
        self.g = SB.BevGenerator(blend=blend, balance=balance, rig=W.rig_s(), output_pitch="auto", input_format=fmt, output_format=out)
        self.batch, self.out = batch, out
        self.d_in = AB.replicated(unique, batch)
        self.d_out = _ffi.DeviceBuffer(batch * self.g.out_image_bytes)
        self.sync, self.tstart, self.tstop = self.g.sync, self.g.timer_start, self.g.timer_stop
        self.tmark, self.tbetween = self.g.timer_mark, self.g.timer_between

    def step(self):
        self.g.run_device(self.d_in.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        """Image b as a BGR array, or as the dense NV12 array of an NV12 handle."""
        c = W.CONFIG_S
        if self.out == "nv12":
            raw = self.d_out.download((self.g.out_image_bytes,), offset=b * self.g.out_image_bytes)
            return SO.from_device(raw, c["BEV_WIDTH"], c["BEV_HEIGHT"], self.g.out_pitch)
        return self.d_out.download((c["BEV_HEIGHT"], self.g.out_pitch, 3), offset=b * self.g.out_image_bytes)[:, :c["BEV_WIDTH"]]


def ab(name, runs, a, frame_texels):
    for r in runs.values():
        for _ in range(a.warmup):
            r.step()
        r.sync()
    # outputs first: the YUYV handle against the BGR handle on the converted frames
    same = all(np.array_equal(runs["bgr"].fetch(b), runs["yuyv"].fetch(b)) for b in (0, min(17, runs["bgr"].batch - 1)))
    laps = {k: [] for k in runs}
    rounds = {k: [] for k in runs}
    names = list(runs)
    for k in range(a.rounds):
        for fmt in (names if k % 2 == 0 else names[::-1]):
            t = AB.timed(runs[fmt], a.steps)
            laps[fmt] += t
            rounds[fmt].append(statistics.median(t))
    med = {k: statistics.median(v) for k, v in laps.items()}
    batch = runs["bgr"].batch
    convert_ms = batch * frame_texels * 5 / (a.copy_gbs * 1e9) * 1e3   # 2 bytes read + 3 written per texel at the copy kernel's rate
    r = {"workload": name, "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps,
         "ms_per_step": {k: round(v, 5) for k, v in med.items()}, "round_medians_ms": {k: [round(x, 5) for x in v] for k, v in rounds.items()},
         "yuyv_over_nv12": round(med["yuyv"] / med["nv12"], 4), "yuyv_over_bgr": round(med["yuyv"] / med["bgr"], 4),
         "convert_pass_ms_at_copy_rate": round(convert_ms, 5), "bgr_plus_convert_ms": round(med["bgr"] + convert_ms, 5),
         "yuyv_below_bgr_plus_convert": bool(med["yuyv"] < med["bgr"] + convert_ms), "outputs_identical": bool(same)}
    if name in ALG:
        r["algorithmic_bytes_per_set"] = ALG[name]
        r["algorithmic_gbs"] = {k: round(b * batch / (med[k] * 1e-3) / 1e9, 1) for k, b in ALG[name].items()}
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workloads", default="config3,config3_nv12out,config4,undistort")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--unique", type=int, default=16, help="distinct frame sets, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    a = p.parse_args()
    _ffi.require_device()
    a.copy_gbs = _ffi.device_copy_rate()
    print(json.dumps({"copy_kernel_gbs_moved": round(a.copy_gbs, 1)}), flush=True)
    rng = np.random.default_rng(a.seed)
    out = []
    for name in a.workloads.split(","):
        if name in ("config3", "config3_nv12out", "config4"):
            c = W.CONFIG_S
            fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
            yu = S.random_yuv422(rng, (a.unique, 4), fw, fh)
            nv = SN.random_nv12(rng, (a.unique, 4), fw, fh)
            blend = balance = name == "config4"
            o = "nv12" if name == "config3_nv12out" else "bgr"
            runs = {"bgr": Stitch("bgr", S.yuv422_to_bgr(yu, "yuyv"), 256, blend, balance, o), "nv12": Stitch("nv12", nv, 256, blend, balance, o),
                    "yuyv": Stitch("yuyv", yu, 256, blend, balance, o)}
            texels = 4 * fw * fh
        elif name == "undistort":
            c = W.CONFIG_UNDISTORT
            fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
            yu = S.random_yuv422(rng, (a.unique,), fw, fh)
            nv = SN.random_nv12(rng, (a.unique,), fw, fh)
            runs = {"bgr": AB.Remap("bgr", S.yuv422_to_bgr(yu, "yuyv"), 64), "nv12": AB.Remap("nv12", nv, 64), "yuyv": AB.Remap("yuyv", yu, 64)}
            texels = fw * fh
        else:
            raise SystemExit("unknown workload %s" % name)
        r = ab(name, runs, a, texels)
        print(json.dumps(r), flush=True)
        out.append(r)
        for run in runs.values():
            run.d_in.free()
            run.d_out.free()
    c3 = [r for r in out if r["workload"] == "config3"]
    print(json.dumps({"summary": {r["workload"]: {"yuyv_over_nv12": r["yuyv_over_nv12"], "yuyv_over_bgr": r["yuyv_over_bgr"]} for r in out},
                      "config3_yardstick_a_1_05": (c3[0]["yuyv_over_nv12"] <= 1.05) if c3 else None,
                      "config3_yardstick_b": c3[0]["yuyv_below_bgr_plus_convert"] if c3 else None,
                      "all_outputs_identical": all(r["outputs_identical"] for r in out)}), flush=True)


if __name__ == "__main__":
    main()
