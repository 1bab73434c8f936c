#!/usr/bin/env python3
"""A/B of the nearest-neighbour one-channel remapper (bevw_remapper_set_interpolation: Undistorter(channels=1, interpolation='nearest'))
against the LINEAR one-channel remapper of ANOTHER build of the library -- the parent commit's -- loaded beside the current one, in ONE
process.

At the geometry of workloads.CONFIG_UNDISTORT and batches 64 and 256, on device-resident buffers, fisheye remappers over the same maps, at
8 and at 16 bits:
  (a) nn<depth>_units       the nearest step of this build on `--unique` seeded label frames (replicated over the batch);
  (b) nn<depth>_per_pixel   the same remapper with the destination 2 bytes off a 4-byte boundary: the per-pixel kernel;
  (c) lin<depth>_parent     the linear one-channel step of `--parent-lib` at that depth on random texels: the bar's reference;
  (d) lin<depth>            the linear step of this build beside (c): the A/B of k_units_gray / k_units_gray16 wherever the two builds' code differs;
  (e) nn<depth>_parent      where `--parent-lib` has the nearest mode: its nearest step on (a)'s frames, beside (a).
Before any timing (a)'s and (b)'s first image is compared with the NumPy statement of cv2's rule and the path of every remapper is read
(bevw_remapper_last_path).  After a warm-up of every shape the variants alternate (order reversed every round) over `--rounds` rounds of
`--steps` steps; a round of one variant is bracketed by the remapper's event timer, and the median over the rounds of the ms per step is
reported with the relative spread (max - min) / median of every variant.

    python tools/nearest_ab.py --parent-lib <libbevwarp.so of the parent commit> [--batches 64,256] [--rounds 5] [--steps 20] [--warmup 10]

One JSON line per batch.  The bar at each depth: the nearest step moves the linear step's bytes on the same schedule and does less, so
(a) <= (c) x (1 + the relative spread of (c) over the rounds of this run).  The copy kernel's time on (a)'s own bytes (source +
destination, from the shapes; bevw_device_copy_rate) stands beside it."""
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

LABELS = {8: (0, 7, 200, 255), 16: (0, 7, 40000, 65535)}
DTYPE = {8: np.uint8, 16: np.uint16}


def load(path):
    """Another build of the library beside the bound one: the signatures it has."""
    L = C.CDLL(path)
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def want_nn(frame, m1, m2):
    """cv2.remap(frame, m1, m2, cv2.INTER_NEAREST), BORDER_CONSTANT 0, on fixed-point maps: map1 + {fx >= 16, fy >= 16} in a short."""
    sh, sw = frame.shape
    a = m2.astype(np.int64) & 1023
    x = (m1[..., 0].astype(np.int64) + ((a & 31) >= 16) + 32768) % 65536 - 32768
    y = (m1[..., 1].astype(np.int64) + ((a >> 5) >= 16) + 32768) % 65536 - 32768
    ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
    return np.where(ok, frame[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], 0).astype(frame.dtype)


class Step:
    """A fisheye remapper of library L in one channel of `depth` bits, nearest or linear, `batch` frames resident on the device; dst_shift:
    bytes the destination lies off its 4-byte boundary."""

    def __init__(self, L, depth, nearest, frames, batch, dst_shift=0):
        c = W.CONFIG_UNDISTORT
        K, D = W.undistort_calibration()
        self.L, self.depth, self.batch = L, depth, batch
        self.r = C.c_void_p()
        self.check(L.bevw_fisheye_remapper_create(0, c["FRAME_WIDTH"], c["FRAME_HEIGHT"], _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(D, 4)),
                                                  float(c["FOCAL_SCALE"]), float(c["SIZE_SCALE"]), 0.0, 0.0, C.byref(self.r)))
        self.check(L.bevw_remapper_set_channels(self.r, 1))
        if depth == 16:
            self.check(L.bevw_remapper_set_depth(self.r, 16))
        if nearest:
            self.check(L.bevw_remapper_set_interpolation(self.r, _ffi.INTER_NEAREST))
        dims = np.zeros(4, np.int32)
        self.check(L.bevw_remapper_dims(self.r, _ffi.ptr(dims)))
        self.out_w, self.out_h = int(dims[2]), int(dims[3])
        reps = np.ascontiguousarray(frames[np.arange(batch) % frames.shape[0]])
        self.src_bytes, self.dst_bytes = reps.nbytes, batch * self.out_w * self.out_h * (depth // 8)
        self.d_in, self.d_out = C.c_void_p(), C.c_void_p()
        self.check(L.bevw_malloc(0, self.src_bytes, C.byref(self.d_in)))
        self.check(L.bevw_malloc(0, self.dst_bytes + 8, C.byref(self.d_out)))
        self.check(L.bevw_memcpy_h2d(0, self.d_in, _ffi.ptr(reps), reps.nbytes))
        self.dst = self.d_out.value + dst_shift

    def check(self, status):
        if status != 0:
            raise RuntimeError(self.L.bevw_last_error().decode("utf-8", "replace"))

    def step(self):
        self.check(self.L.bevw_remap_device(self.r, self.d_in, self.batch, self.dst))

    def sync(self):
        self.check(self.L.bevw_remapper_sync(self.r))

    def timed(self, steps):
        """ms per step of `steps` steps between two events on the remapper's stream"""
        ms = C.c_float()
        self.check(self.L.bevw_remapper_timer_start(self.r))
        for _ in range(steps):
            self.step()
        self.check(self.L.bevw_remapper_timer_stop(self.r, C.byref(ms)))
        return ms.value / steps

    def fetch(self, b):
        out = np.empty((self.out_h, self.out_w), DTYPE[self.depth])
        self.sync()
        self.check(self.L.bevw_memcpy_d2h(0, _ffi.ptr(out), self.dst + b * out.nbytes, out.nbytes))
        return out

    def maps(self):
        m1, m2 = np.empty((self.out_h, self.out_w, 2), np.int16), np.empty((self.out_h, self.out_w), np.uint16)
        self.check(self.L.bevw_remapper_get_maps(self.r, _ffi.ptr(m1), _ffi.ptr(m2)))
        return m1, m2

    def close(self):
        self.L.bevw_remapper_destroy(self.r)
        self.L.bevw_free(0, self.d_in)
        self.L.bevw_free(0, self.d_out)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--parent-lib", required=True, help="libbevwarp.so built from the parent commit")
    p.add_argument("--batches", default="64,256")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--unique", type=int, default=16, help="distinct frames, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    a = p.parse_args()
    _ffi.require_device()
    L, P = _ffi.lib(), load(a.parent_lib)
    c = W.CONFIG_UNDISTORT
    fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
    rng = np.random.default_rng(a.seed)
    labels = {d: np.asarray(LABELS[d], DTYPE[d])[rng.integers(0, 4, (a.unique, fh, fw))] for d in (8, 16)}
    noise = {d: rng.integers(0, 1 << d, (a.unique, fh, fw), dtype=DTYPE[d]) for d in (8, 16)}
    out = []
    for batch in (int(b) for b in a.batches.split(",")):
        r = {"workload": "undistort", "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps}
        for d in (8, 16):
            nn, pp, par, lin = "nn%d_units" % d, "nn%d_per_pixel" % d, "lin%d_parent" % d, "lin%d" % d
            runs = {nn: Step(L, d, True, labels[d], batch), pp: Step(L, d, True, labels[d], batch, dst_shift=2),
                    par: Step(P, d, False, noise[d], batch), lin: Step(L, d, False, noise[d], batch)}
            if hasattr(P, "bevw_remapper_set_interpolation"):
                runs["nn%d_parent" % d] = Step(P, d, True, labels[d], batch)
            for run in runs.values():
                for _ in range(a.warmup):
                    run.step()
                run.sync()
            paths = {k: int(run.L.bevw_remapper_last_path(run.r)) for k, run in runs.items()}
            want = want_nn(labels[d][0], *runs[nn].maps())
            same = {k: bool(np.array_equal(runs[k].fetch(0), want)) for k in (nn, pp)}
            laps, names = {k: [] for k in runs}, list(runs)
            for k in range(a.rounds):
                for name in (names if k % 2 == 0 else names[::-1]):
                    laps[name].append(runs[name].timed(a.steps))
            med = {k: statistics.median(v) for k, v in laps.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in laps.items()}
            u = runs[nn]
            step_bytes = u.src_bytes + u.dst_bytes
            g = C.c_double()
            u.check(L.bevw_device_copy_rate(0, step_bytes // 2 // 16 * 16, 10, 0, C.byref(g)))   # (a copy READS and WRITES its size: half the step's bytes each way)
            bar = med[par] * (1.0 + spread[par])
            r["depth_%d" % d] = {
                "paths": paths, "ms_per_step": {k: round(v, 5) for k, v in med.items()}, "rounds_ms": {k: [round(x, 5) for x in v] for k, v in laps.items()},
                "relative_spread": {k: round(v, 4) for k, v in spread.items()}, "nearest_over_parent_linear": round(med[nn] / med[par], 4),
                "bar_ms": round(bar, 5), "bar_met": bool(med[nn] <= bar), "missed_by": round(max(0.0, med[nn] / bar - 1.0), 4),
                "bytes_src_plus_dst": step_bytes, "nearest_gbs": round(step_bytes / (med[nn] * 1e-3) / 1e9, 1), "copy_kernel_gbs_moved": round(g.value, 1),
                "copy_kernel_ms_on_the_same_bytes": round(step_bytes / (g.value * 1e9) * 1e3, 5), "equals_the_statement": same,
                "units": paths[nn] == _ffi.PATH_UNITS and paths[par] == _ffi.PATH_UNITS, "per_pixel": paths[pp] == _ffi.PATH_PER_PIXEL}
            for run in runs.values():
                run.close()
        print(json.dumps(r), flush=True)
        out.append(r)
    cells = [(r["batch"], d, r["depth_%d" % d]) for r in out for d in (8, 16)]
    print(json.dumps({"summary": {"%d/%d" % (b, d): x["nearest_over_parent_linear"] for b, d, x in cells}, "bar_met": all(x["bar_met"] for _, _, x in cells),
                      "units": all(x["units"] for _, _, x in cells), "per_pixel": all(x["per_pixel"] for _, _, x in cells),
                      "all_equal_the_statement": all(all(x["equals_the_statement"].values()) for _, _, x in cells)}), flush=True)


if __name__ == "__main__":
    main()
