#!/usr/bin/env python3
"""A/B of NV12 surfaces read in place (bevw_run_surface_table_device, bevw_remap_surfaces_device) against the packed NV12 layout, in ONE process.

Variants, all device-resident, the same seeded frames (`--unique` frame sets replicated over the batch):
  P    packed: run_device on [B][4][FH*3/2][FW] -- the baseline;
  S0   surfaces over the very same bytes: pitch FW, uv = y + FW*FH, the table points into P's buffer -- what the indirection costs;
  S1   surfaces as a decoder leaves them: pitch `--pitch` (1536), one pool per camera, the surfaces of a pool in shuffled order, gaps
       between the planes;
  C+P  what a user had to do before: a device copy that packs S1-shaped surfaces into the dense layout, then P.  The copy is a yardstick,
       not product code, measured two ways (pack_copy_ms): one hipMemcpy2DAsync per surface through ctypes, and the floor the library's
       own copy kernel sets for the same bytes; C+P is the SUM of the copy and P's median (the step depends on the copy: no overlap), and
       the bar S1 < C+P is taken against the faster of the two copies.
After a warm-up the handles alternate (order rotated every round) over `--rounds` rounds of `--steps` timed steps; every step is bracketed
by the handle's timer marks, and the median ms per step of each variant is reported.  S0 and S1 must return P's bytes (two frame sets).

    python tools/nv12_surfaces_ab.py [--workloads config3,config3_nv12out,config4,undistort] [--rounds 5] [--steps 20] [--warmup 10]

One JSON line per workload, then a summary with the bars: S0 / P <= 1.05, S1 / S0 <= 1.05, S1 < C+P.  Kernel names of a surface step: run
under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/nv12_surfaces_ab.py --workloads config3 --only S1 --rounds 1 --steps 1
--warmup 0` (a run of its own) -- no copy or pack kernel may appear."""
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


def pitched(frame: np.ndarray, fh: int, pitch: int, rng):
    """NV12 frame [fh*3//2, fw] -> (Y plane [fh, pitch], U/V plane [fh//2, pitch]) with random padding columns."""
    fw = frame.shape[1]
    y = rng.integers(0, 256, (fh, pitch), dtype=np.uint8)
    uv = rng.integers(0, 256, (fh // 2, pitch), dtype=np.uint8)
    y[:, :fw], uv[:, :fw] = frame[:fh], frame[fh:]
    return y, uv


class Pools:
    """S1: per camera one device pool of `batch` surfaces in shuffled order, every plane behind a gap of its own."""

    def __init__(self, unique, batch, ncams, fw, fh, pitch, rng):
        ysz, csz, gap = pitch * fh, pitch * fh // 2, 4096
        slot = ysz + csz + 2 * gap
        self.bufs, table = [], np.zeros((batch, ncams, 2), np.uint64)
        for c in range(ncams):
            buf = _ffi.DeviceBuffer(slot * batch + gap)
            order = rng.permutation(batch)
            planes = [pitched(unique[u, c] if ncams > 1 else unique[u], fh, pitch, rng) for u in range(len(unique))]
            for b in range(batch):
                y, uv = planes[b % len(unique)]
                base = gap + int(order[b]) * slot
                yo, co = (base, base + ysz + gap) if b % 2 == 0 else (base + csz + gap, base)   # U/V above or below Y
                buf.upload(y, yo)
                buf.upload(uv, co)
                table[b, c] = (buf.ptr + yo, buf.ptr + co)
            self.bufs.append(buf)
        self.table = table

    def free(self):
        for b in self.bufs:
            b.free()


class Stitch:
    def __init__(self, variant, unique, batch, blend, balance, out_fmt, pitch, rng, shared_in=None):
        from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB

        c = W.CONFIG_S
        fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
        ns = SB.BevGenerator.get_args()
        for k, v in c.items():
            setattr(ns, k, v)
        self.variant, self.batch, self.pools, self.d_in = variant, batch, None, None
        self.g = SB.BevGenerator(blend=blend, balance=balance, rig=W.rig_s(), output_pitch="auto", input_format="nv12", output_format=out_fmt,
                                 input_pitch=pitch if variant == "S1" else None)
        if variant == "P":
            self.d_in = _ffi.DeviceBuffer(batch * unique[0].nbytes)
            for b in range(batch):
                self.d_in.upload(unique[b % len(unique)], b * unique[0].nbytes)
        elif variant == "S0":   # the table points into P's buffer
            base = shared_in.ptr + np.arange(batch * 4, dtype=np.uint64).reshape(batch, 4) * np.uint64(fw * fh * 3 // 2)
            table = np.stack([base, base + np.uint64(fw * fh)], axis=-1)
        else:
            self.pools = Pools(unique, batch, 4, fw, fh, pitch, rng)
            table = self.pools.table
        if variant != "P":
            self.d_table = _ffi.DeviceBuffer(table.nbytes).upload(np.ascontiguousarray(table, np.uint64))
        self.d_out = _ffi.DeviceBuffer(batch * self.g.out_image_bytes)
        self.sync, self.tstart, self.tstop = self.g.sync, self.g.timer_start, self.g.timer_stop
        self.tmark, self.tbetween = self.g.timer_mark, self.g.timer_between

    def step(self):
        if self.variant == "P":
            self.g.run_device(self.d_in.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)
        else:
            self.g.run_surface_table(self.d_table.ptr, self.batch, None, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        return self.d_out.download((self.g.out_image_bytes,), offset=b * self.g.out_image_bytes)

    def free(self):
        for x in (self.d_in, getattr(self, "d_table", None), self.d_out, self.pools):
            if x is not None:
                x.free()


class Remap:
    def __init__(self, variant, unique, batch, pitch, rng, shared_in=None):
        from cameracalibration_amd.Tools import undistort as U

        c = W.CONFIG_UNDISTORT
        fw, fh = c["FRAME_WIDTH"], c["FRAME_HEIGHT"]
        K, D = W.undistort_calibration()
        self.variant, self.batch, self.pools, self.d_in = variant, batch, None, None
        self.u = U.Undistorter(K, D, fw, fh, focalscale=c["FOCAL_SCALE"], sizescale=c["SIZE_SCALE"], input_format="nv12",
                               input_pitch=pitch if variant == "S1" else None)
        self.r, L = self.u._r, _ffi.lib()
        if variant == "P":
            self.d_in = _ffi.DeviceBuffer(batch * unique[0].nbytes)
            for b in range(batch):
                self.d_in.upload(unique[b % len(unique)], b * unique[0].nbytes)
        elif variant == "S0":
            base = shared_in.ptr + np.arange(batch, dtype=np.uint64) * np.uint64(fw * fh * 3 // 2)
            self.table = np.ascontiguousarray(np.stack([base, base + np.uint64(fw * fh)], axis=-1), np.uint64)
        else:
            self.pools = Pools(unique, batch, 1, fw, fh, pitch, rng)
            self.table = np.ascontiguousarray(self.pools.table[:, 0], np.uint64)
        if variant != "P":
            self.d_table = _ffi.DeviceBuffer(self.table.nbytes).upload(self.table)
        self.d_out = _ffi.DeviceBuffer(batch * self.u.out_image_bytes)
        self.sync = self.u.sync
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
        if self.variant == "P":
            _ffi.check(_ffi.lib().bevw_remap_device(self.r, self.d_in.ptr, self.batch, self.d_out.ptr))
        else:
            self.u.run_surface_table(self.d_table.ptr, self.batch, self.d_out.ptr, out_bytes=self.d_out.nbytes)

    def fetch(self, b):
        return self.d_out.download((self.u.out_image_bytes,), offset=b * self.u.out_image_bytes)

    def free(self):
        for x in (self.d_in, getattr(self, "d_table", None), self.d_out, self.pools):
            if x is not None:
                x.free()
        self.u.close()


def timed(run, steps):
    run.tstart()
    for i in range(steps):
        run.tmark(i)
        run.step()
    run.tmark(steps)
    run.tstop()
    return [run.tbetween(i, i + 1) for i in range(steps)]


def pack_copy_ms(batch, ncams, fw, fh, pitch, steps, warmup):
    """The yardstick copy C: S1-shaped surfaces (rows of `pitch` bytes, one pool per camera) -> the dense layout, measured two ways.
    "memcpy2d": what a user of the runtime writes -- one hipMemcpy2DAsync per surface (Y and U / V rows in one call: the yardstick's
    surfaces keep U / V right behind Y), batch * ncams calls per step, wall time per step around a device synchronisation.
    "kernel_floor": the same bytes at the rate of the library's own copy kernel (bevw_device_copy_rate over a buffer of the packed
    batch's size): bytes read + written / rate -- no packing copy can be faster.  Returns (memcpy2d_ms, kernel_floor_ms)."""
    import time
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpy2DAsync.restype = C.c_int
    rows, frame = fh * 3 // 2, fw * fh * 3 // 2
    pools = [_ffi.DeviceBuffer(batch * rows * pitch) for _ in range(ncams)]
    dst = _ffi.DeviceBuffer(batch * ncams * frame)

    def step():
        for b in range(batch):
            for c in range(ncams):
                e = hip.hipMemcpy2DAsync(dst.ptr + (b * ncams + c) * frame, fw, pools[c].ptr + b * rows * pitch, pitch, fw, rows, 3, None)
                if e != 0:
                    raise SystemExit("hipMemcpy2DAsync failed: %d" % e)
    for _ in range(min(warmup, 2)):
        step()
    hip.hipDeviceSynchronize()
    t = []
    for _ in range(max(3, steps // 4)):
        t0 = time.perf_counter()
        step()
        hip.hipDeviceSynchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    for b in pools + [dst]:
        b.free()
    moved = 2.0 * batch * ncams * frame   # bytes read + written
    rate = _ffi.device_copy_rate(batch * ncams * frame, reps=10)   # GB/s moved
    return statistics.median(t), moved / (rate * 1e9) * 1e3


def ab(name, runs, a, copy_ms):
    for r in runs.values():
        for _ in range(a.warmup):
            r.step()
        r.sync()
    laps, rounds, names = {k: [] for k in runs}, {k: [] for k in runs}, list(runs)
    for k in range(a.rounds):
        for v in names[k % len(names):] + names[:k % len(names)]:
            t = timed(runs[v], a.steps)
            laps[v] += t
            rounds[v].append(statistics.median(t))
    med = {k: statistics.median(v) for k, v in laps.items()}
    batch = next(iter(runs.values())).batch
    same = all(np.array_equal(runs["P"].fetch(b), runs[v].fetch(b)) for v in runs if v != "P" for b in (0, min(17, batch - 1))) if "P" in runs else None
    out = {"workload": name, "batch": batch, "rounds": a.rounds, "steps_per_round": a.steps, "input_pitch_S1": a.pitch,
           "ms_per_step": {k: round(v, 5) for k, v in med.items()}, "round_medians_ms": {k: [round(x, 5) for x in v] for k, v in rounds.items()},
           "outputs_identical": same,
           "pack_copy_ms": None if copy_ms is None else {"memcpy2d": round(copy_ms[0], 5), "kernel_floor": round(copy_ms[1], 5)}}
    if "P" in med and "S0" in med:
        out["S0_over_P"] = round(med["S0"] / med["P"], 4)
    if "S1" in med and "S0" in med:
        out["S1_over_S0"] = round(med["S1"] / med["S0"], 4)
    if copy_ms is not None and "P" in med and "S1" in med:   # the bar takes the FASTER copy: the floor no packing copy can beat
        out["C_plus_P_ms"] = {"memcpy2d": round(copy_ms[0] + med["P"], 5), "kernel_floor": round(copy_ms[1] + med["P"], 5)}
        out["S1_over_C_plus_P"] = round(med["S1"] / (min(copy_ms) + med["P"]), 4)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workloads", default="config3,config3_nv12out,config4,undistort")
    p.add_argument("--only", default="P,S0,S1", help="variants to run")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--pitch", type=int, default=1536, help="row pitch of S1's surfaces (the undistort workload: its width rounded up to 256, + 256)")
    p.add_argument("--unique", type=int, default=16, help="distinct frame sets, replicated over the batch")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--no-copy", action="store_true", help="skip the packing-copy yardstick")
    a = p.parse_args()
    _ffi.require_device()
    rng = np.random.default_rng(a.seed)
    want = a.only.split(",")
    out = []
    for name in a.workloads.split(","):
        runs = {}
        if name in ("config3", "config3_nv12out", "config4"):
            c = W.CONFIG_S
            fw, fh, batch, ncams, pitch = c["FRAME_WIDTH"], c["FRAME_HEIGHT"], 256, 4, a.pitch
            nv = S.random_nv12(rng, (a.unique, 4), fw, fh)
            blend = balance = name == "config4"
            fmt = "nv12" if name == "config3_nv12out" else "bgr"
            if "P" in want or "S0" in want:
                runs["P"] = Stitch("P", nv, batch, blend, balance, fmt, pitch, rng)
            if "S0" in want:
                runs["S0"] = Stitch("S0", nv, batch, blend, balance, fmt, pitch, rng, shared_in=runs["P"].d_in)
            if "S1" in want:
                runs["S1"] = Stitch("S1", nv, batch, blend, balance, fmt, pitch, rng)
        elif name == "undistort":
            c = W.CONFIG_UNDISTORT
            fw, fh, batch, ncams = c["FRAME_WIDTH"], c["FRAME_HEIGHT"], 64, 1
            pitch = (fw + 255) // 256 * 256 + 256
            nv = S.random_nv12(rng, (a.unique,), fw, fh)
            if "P" in want or "S0" in want:
                runs["P"] = Remap("P", nv, batch, pitch, rng)
            if "S0" in want:
                runs["S0"] = Remap("S0", nv, batch, pitch, rng, shared_in=runs["P"].d_in)
            if "S1" in want:
                runs["S1"] = Remap("S1", nv, batch, pitch, rng)
        else:
            raise SystemExit("unknown workload %s" % name)
        copy_ms = None if a.no_copy else pack_copy_ms(batch, ncams, fw, fh, pitch, a.steps, a.warmup)
        r = ab(name, runs, a, copy_ms)
        print(json.dumps(r), flush=True)
        out.append(r)
        for run in runs.values():
            run.free()
    def bar(key, ok):   # None when no workload produced the figure: a bar that was not evaluated is not a bar that was met
        v = [r[key] for r in out if r.get(key) is not None]
        return all(ok(x) for x in v) if v else None
    print(json.dumps({"summary": {r["workload"]: {k: r.get(k) for k in ("S0_over_P", "S1_over_S0", "S1_over_C_plus_P")} for r in out},
                      "bar_S0_over_P_1_05": bar("S0_over_P", lambda x: x <= 1.05),
                      "bar_S1_over_S0_1_05": bar("S1_over_S0", lambda x: x <= 1.05),
                      "bar_S1_below_C_plus_P": bar("S1_over_C_plus_P", lambda x: x < 1.0),
                      "all_outputs_identical": all(r["outputs_identical"] for r in out if r["outputs_identical"] is not None)}), flush=True)


if __name__ == "__main__":
    main()
