#!/usr/bin/env python3
"""A/B of NV12 BEV output (bevw_set_output_format) against BGR output, in ONE process.

Per workload, handles of every format pair below are built on the same rig and fed the same seeded frames (`--unique` random frame sets
replicated over the batch in device memory; NV12 frames for NV12 input, their conversion by tests/_nv12_spec.py for BGR input).  After a
warm-up the handles alternate (order rotated every round) over `--rounds` rounds of `--steps` timed steps on device-resident buffers; every
step is bracketed by the handle's timer marks.  Reported per handle: the median ms per step, its ratio to BGR -> BGR, and the roofline
fraction of its algorithmic bytes (HBM spec peak 8 TB/s, as bench.py).  Each NV12 result must equal the NumPy spec applied to the BGR
handle's result (checked on two frame sets).

    python tools/nv12_out_ab.py [--workloads config3,config4,undistort] [--rounds 6] [--steps 20] [--warmup 10]

Workloads (in -> out): config3 = BASELINE config 3 (1280 x 960 -> 1080 x 1080 direct, batch 256, pitched device images): bgr->bgr,
bgr->nv12, nv12->nv12; config4 = blend + balance on the same rig: bgr->bgr, bgr->nv12; undistort = BASELINE config 2 (fisheye remap,
batch 64): bgr->bgr, bgr->nv12.  One JSON line per workload, then a summary line; the bar of the feature is config3 bgr->nv12 / bgr->bgr
<= 1.  Kernel times: `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/nv12_out_ab.py ...` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cameracalibration_amd import _ffi, workloads as W  # noqa: E402
from nv12_ab import Remap, Stitch, replicated, timed  # noqa: E402
from tests import _nv12_out_spec as SO  # noqa: E402
from tests import _nv12_spec as S  # noqa: E402

HBM_PEAK_GBS = 8000.0
# algorithmic bytes per frame set: source bytes touched (workloads.ALGORITHMIC_BYTES; NV12 frames 1.5 bytes per touched texel) + output bytes
# (BGR 3, NV12 1.5 per pixel).  config 4 also reads every frame byte once for the V means.
ALG = {
    "config3": {"bgr>bgr": 2_033_157 + 3_499_200, "bgr>nv12": 2_033_157 + 1_749_600, "nv12>nv12": 2_033_157 // 2 + 1_749_600},
    "config4": {"bgr>bgr": 14_745_600 + 2 * 2_170_338 + 3_499_200, "bgr>nv12": 14_745_600 + 2 * 2_170_338 + 1_749_600},
    "undistort": {"bgr>bgr": 1_735_512 + 3_686_400, "bgr>nv12": 1_735_512 + 1_843_200},
}


class StitchOut(Stitch):
    """nv12_ab.Stitch with an output format"""

    def __init__(self, fmt_in, fmt_out, unique, batch, blend, balance):
        from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

        ns = SB.BevGenerator.get_args()
        for k, v in W.CONFIG_S.items():
            setattr(ns, k, v)
        self.g = SB.BevGenerator(blend=blend, balance=balance, rig=W.rig_s(), output_pitch="auto", input_format=fmt_in, output_format=fmt_out)
        self.fmt_out, self.batch = fmt_out, batch
        self.d_in = replicated(unique, batch)
        self.d_out = _ffi.DeviceBuffer(batch * self.g.out_image_bytes)
        self.sync, self.tstart, self.tstop = self.g.sync, self.g.timer_start, self.g.timer_stop
        self.tmark, self.tbetween = self.g.timer_mark, self.g.timer_between

    def fetch(self, b):
        c = W.CONFIG_S
        if self.fmt_out == "nv12":
            raw = self.d_out.download((self.g.out_image_bytes,), offset=b * self.g.out_image_bytes)
            return SO.from_device(raw, c["BEV_WIDTH"], c["BEV_HEIGHT"], self.g.out_pitch)
        return super().fetch(b)


class RemapOut(Remap):
    """nv12_ab.Remap with an output format"""

    def __init__(self, fmt_in, fmt_out, unique, batch):
        super().__init__(fmt_in, unique, batch)
        self.fmt_out = fmt_out
        if fmt_out == "nv12":
            _ffi.check(_ffi.lib().bevw_remapper_set_output_format(self.r, _ffi.OUTPUT_NV12))
            self.u.output_format = "nv12"
            self.img = self.u.out_w * self.u.out_h * 3 // 2

    def fetch(self, b):
        if self.fmt_out == "nv12":
            return self.d_out.download((self.u.out_h * 3 // 2, self.u.out_w), offset=b * self.img)
        return super().fetch(b)


def ab(name, runs, a):
    for r in runs.values():
        for _ in range(a.warmup):
            r.step()
        r.sync()
    laps = {k: [] for k in runs}
    rounds = {k: [] for k in runs}
    names = list(runs)
    for k in range(a.rounds):
        order = names[k % len(names):] + names[:k % len(names)]
        for fmt in (order if k % 2 == 0 else order[::-1]):
            t = timed(runs[fmt], a.steps)
            laps[fmt] += t
            rounds[fmt].append(statistics.median(t))
    base = runs["bgr>bgr"]
    same = True
    for b in (0, min(17, base.batch - 1)):
        want = base.fetch(b)
        for k, r in runs.items():
            got = r.fetch(b)
            same = same and np.array_equal(got, SO.bgr_to_nv12(want) if k.endswith("nv12") else want)
    med = {k: statistics.median(v) for k, v in laps.items()}
    gbs = {k: ALG[name][k] * runs[k].batch / (med[k] * 1e-3) / 1e9 for k in runs}
    return {"workload": name, "batch": base.batch, "rounds": a.rounds, "steps_per_round": a.steps,
            "ms_per_step": {k: round(v, 5) for k, v in med.items()},
            "round_medians_ms": {k: [round(x, 5) for x in v] for k, v in rounds.items()},
            "over_bgr_bgr": {k: round(med[k] / med["bgr>bgr"], 4) for k in runs},
            "algorithmic_bytes_per_set": ALG[name],
            "algorithmic_gbs": {k: round(v, 1) for k, v in gbs.items()},
            "roofline_frac": {k: round(v / HBM_PEAK_GBS, 4) for k, v in gbs.items()},
            "outputs_match_spec": bool(same)}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workloads", default="config3,config4,undistort")
    p.add_argument("--rounds", type=int, default=6)
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
            runs = {"bgr>bgr": StitchOut("bgr", "bgr", bgr, 256, blend, balance), "bgr>nv12": StitchOut("bgr", "nv12", bgr, 256, blend, balance)}
            if name == "config3":
                runs["nv12>nv12"] = StitchOut("nv12", "nv12", nv, 256, blend, balance)
        elif name == "undistort":
            c = W.CONFIG_UNDISTORT
            bgr = S.nv12_to_bgr(S.random_nv12(rng, (a.unique,), c["FRAME_WIDTH"], c["FRAME_HEIGHT"]))
            runs = {"bgr>bgr": RemapOut("bgr", "bgr", bgr, 64), "bgr>nv12": RemapOut("bgr", "nv12", bgr, 64)}
        else:
            raise SystemExit("unknown workload %s" % name)
        r = ab(name, runs, a)
        print(json.dumps(r), flush=True)
        out.append(r)
        for run in runs.values():
            run.d_in.free()
            run.d_out.free()
    c3 = [r for r in out if r["workload"] == "config3"]
    print(json.dumps({"summary": {r["workload"]: r["over_bgr_bgr"] for r in out},
                      "config3_bar_bgr_nv12_le_1": (c3[0]["over_bgr_bgr"]["bgr>nv12"] <= 1.0) if c3 else None,
                      "all_outputs_match_spec": all(r["outputs_match_spec"] for r in out)}), flush=True)


if __name__ == "__main__":
    main()
