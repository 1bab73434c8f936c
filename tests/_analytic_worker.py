"""Worker of tests/test_analytic_gpu.py: one fresh process per setting of BEVW_ANALYTIC_UNITS / BEVW_ANALYTIC_FRAMES (the library reads
them once per process).

argv: case_dir.  The parent sets the switches in this process's environment and leaves jobs.json in case_dir: a list of
{name, rig, cfg, blend, balance, projection, frames: <file>.npy, car: bool}.  Every job stitches its frames through a fresh
BevGenerator into a buffer filled with 0x5A (run_device) and leaves got_<name>.npy and, in info.json, the handle's plan_info() after the run.  The parent compares with the
specification: nothing is judged here."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    case_dir = sys.argv[1]
    from tests import _analytic_common as AC
    from tests._harness import set_args, worker_library

    ffi, SB = worker_library({})
    jobs = json.load(open(os.path.join(case_dir, "jobs.json")))
    info = {}
    for j in jobs:
        set_args(SB, j["cfg"])
        bev = SB.BevGenerator(blend=j["blend"], balance=j["balance"], rig=AC.RIGS[j["rig"]](), projection=j["projection"])
        frames = np.load(os.path.join(case_dir, j["frames"]))
        got = AC.stitch_filled(ffi, bev, frames, AC.make_car(j["cfg"]) if j["car"] else None)
        np.save(os.path.join(case_dir, "got_%s.npy" % j["name"]), got)
        info[j["name"]] = bev.plan_info()
        print("ran", j["name"], info[j["name"]], flush=True)
    json.dump(info, open(os.path.join(case_dir, "info.json"), "w"))
    print("worker OK", flush=True)


if __name__ == "__main__":
    main()
