"""Build recipe of libbevwarp.so (hipcc, gfx950 only).  Used by __graft_entry__.build() and by hand:

    python -m cameracalibration_amd.build [--force]

Nine translation units -- bevwarp.hip (handles, table builders, tools, the camera-per-GPU exchange), bevwarp_plan.hip (the tile plan
and its per-frame kernels), bevwarp_jpeg.hip (the JPEG codec), bevwarp_yuv422.hip (every kernel that reads packed 4:2:2 camera frames:
FORMAT_UNITS), bevwarp_gray.hip (every kernel of the one-channel remapper: CHANNEL_UNITS) and bevwarp_gray_stitch.hip (every kernel of the
one-channel stitch: STITCH_CHANNEL_UNITS) and bevwarp_moving.hip (the stitch with a homography per frame set: MOVING_UNITS) and bevwarp_gray16.hip (every kernel of the 16-bit
one-channel remapper: DEPTH_UNITS) and bevwarp_nearest.hip (every kernel of the
nearest-neighbour one-channel remapper: INTERP_UNITS) -- are compiled in parallel into objects under csrc/build/ and linked;
a unit is recompiled when its source, ANY header under csrc/ or the flag set changed.  The shared object is written next to this file (in-tree: it travels
to the GPU box with the repo snapshot and is git-ignored).  -ffp-contract=off is REQUIRED: the arithmetic being reproduced has no fused
multiply-add.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libbevwarp.so")
# translation units; every header under csrc/ (and the public header) is a dependency of every unit: a header edit can never leave a
# stale object behind (round 4's explicit lists had missed bevw_jpeg_walk.h and bevw_device.h for the JPEG unit)
UNITS = ["bevwarp.hip", "bevwarp_plan.hip", "bevwarp_jpeg.hip"]
# units that hold the kernels of one input format and nothing else: the shared device functions of the headers instantiated for that
# format, under kernel names of their own (no kernel of UNITS is compiled a second time)
FORMAT_UNITS = ["bevwarp_yuv422.hip"]
# units that hold the kernels of one channel count: the one-channel remapper (bevw_remapper_set_channels), every kernel named *gray*
CHANNEL_UNITS = ["bevwarp_gray.hip"]
# ... and the one-channel stitch of a handle (bevw_set_channels): the unit kernel over every class, the per-tap and the per-pixel kernel
STITCH_CHANNEL_UNITS = ["bevwarp_gray_stitch.hip"]
ALL_UNITS = UNITS + FORMAT_UNITS + CHANNEL_UNITS + STITCH_CHANNEL_UNITS
# ... and the stitch with a homography per frame set (bevw_run_homographies_device): k_stitch_moving, direct and blend.  A list beside
# ALL_UNITS: the six units above compile to the code objects they were before this one existed
MOVING_UNITS = ["bevwarp_moving.hip"]
BUILD_UNITS = ALL_UNITS + MOVING_UNITS
# ... and the 16-bit one-channel remapper (bevw_remapper_set_depth): every kernel named *gray16*.  A list of its own again: the seven units
# above compile to the code objects they were before this one existed
DEPTH_UNITS = ["bevwarp_gray16.hip"]
LINK_UNITS = BUILD_UNITS + DEPTH_UNITS
# ... and the nearest-neighbour one-channel remapper (bevw_remapper_set_interpolation): every kernel named *nn8* / *nn16*.  A list of its own
# once more: the eight units above compile to the code objects they were before this one existed
INTERP_UNITS = ["bevwarp_nearest.hip"]
LINKED = LINK_UNITS + INTERP_UNITS   # what is compiled and linked


def _headers():
    import glob
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "bevwarp.h")]


CFLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-Wno-pass-failed", "-Wno-inline-asm"]
EXTRA = os.environ.get("BEVW_CFLAGS", "").split()   # experiment builds (e.g. -DBEVW_UNIT_DEPTH=4)
TAG = os.environ.get("BEVW_BUILD_TAG", "")            # ... land in build_var/libbevwarp_<tag>.so (objects in csrc/build_<tag>/); A/B through BEVW_LIB_PATH
if TAG:
    OBJ = os.path.join(CSRC, "build_" + TAG)
    LIB = os.path.join(os.path.dirname(HERE), "build_var", "libbevwarp_%s.so" % TAG)


def _newer(path: str, deps) -> bool:
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if EXTRA and not TAG:
        # experiment flags never land in the default objects / libbevwarp.so (a later plain build would keep them: fresh mtimes)
        raise SystemExit("BEVW_CFLAGS needs BEVW_BUILD_TAG=<tag>: experiment builds go to build_var/libbevwarp_<tag>.so")
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    me = os.path.abspath(__file__)
    # the flag set the objects were compiled with: a different one (another BEVW_CFLAGS under the same tag) rebuilds everything
    stamp, flags = os.path.join(OBJ, "flags.stamp"), " ".join(CFLAGS + EXTRA)
    if not os.path.exists(stamp) or open(stamp).read() != flags:
        force = True
    jobs = []
    hdrs = _headers()
    for src in LINKED:
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        deps = [os.path.join(CSRC, src)] + hdrs + [me]
        if force or _newer(obj, deps):
            jobs.append([hipcc] + CFLAGS + EXTRA + ["-c", os.path.join(CSRC, src), "-o", obj])
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in LINKED]
    if not jobs and not _newer(LIB, objs):
        return LIB

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=len(LINKED)) as pool:
        list(pool.map(run, jobs))
    with open(stamp, "w") as f:
        f.write(flags)
    run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", LIB + ".tmp"])
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
