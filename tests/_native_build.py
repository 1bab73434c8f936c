"""Builds the host-side emulators under tests/native/ with hipcc; runs the unit emulator (run_units) and lists the kernels of a unit's
code object (kernels_of) for the host tests that share them.

Only the HOST half of those files ever runs (the kernels' __host__ __device__ lane code on the CPU), so the device half is not compiled:
`--cuda-host-only` takes seconds instead of the 90 s a gfx950 code object of the plan kernels costs.  A host object of a file with
__global__ kernels still registers a fat binary at start-up; a stub of eight zero bytes under the symbol it asks for satisfies the linker,
and the runtime never looks at it because no kernel is launched.  Falls back to the full build when anything of that fails."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FLAGS = ["-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-pass-failed", "-Wno-inline-asm", "-Wno-unused-result"]


def hipcc_path():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def build(src: str, exe: str, timeout: int = 900, sanitize: bool = False, extra=()) -> None:
    """sanitize: AddressSanitizer + UndefinedBehaviorSanitizer (clang's runtimes ship with ROCm's llvm); any finding aborts the program.
    extra: more compiler flags (e.g. -DBEVW_UNIT_STORE16=2 for the emulator of a variant build)."""
    hipcc = hipcc_path()
    obj, stub_c, stub_o = exe + ".o", exe + "_fatbin_stub.c", exe + "_fatbin_stub.o"
    sanitize = sanitize or os.environ.get("BEVW_NATIVE_SANITIZE") == "1"   # the sanitizer leg re-runs the emulator tests this way
    san = SANITIZE if sanitize else []
    try:
        r = subprocess.run([hipcc] + FLAGS + list(extra) + san + ["--cuda-host-only", "-c", src, "-o", obj], capture_output=True, text=True, timeout=timeout)
        if r.returncode == 0:
            syms = subprocess.run(["nm", obj], capture_output=True, text=True, timeout=60).stdout
            wanted = sorted(set(re.findall(r"^\s+U (__hip_fatbin\w*)$", syms, flags=re.M)))
            with open(stub_c, "w") as f:
                for s in wanted:
                    f.write('__attribute__((section(".hip_fatbin"), aligned(4096))) const char %s[8] = {0};\n' % s)
                f.write("int bevw_native_build_stub;\n")
            ok = subprocess.run(["gcc", "-c", stub_c, "-o", stub_o], capture_output=True, text=True, timeout=60).returncode == 0
            ok = ok and subprocess.run([hipcc] + san + [obj, stub_o, "-o", exe], capture_output=True, text=True, timeout=300).returncode == 0
            if ok and subprocess.run([exe, "--bevw-selfcheck-noop"], capture_output=True, timeout=120).returncode is not None:
                return
    except (OSError, subprocess.SubprocessError):
        pass
    assert not sanitize, "sanitized host build failed: " + (r.stderr[-2000:] if "r" in dir() else "")
    r = subprocess.run([hipcc] + FLAGS + list(extra) + [src, "-o", exe], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]


def kernels_of(obj: str, tmp: str) -> set:
    """Names of the kernels (their kernel descriptors, `<name>.kd`) in the gfx950 code object of a unit's object file."""
    stem = os.path.join(tmp, os.path.basename(obj))
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + stem + ".fatbin", obj, stem + ".host"],
                   check=True, capture_output=True, timeout=120)
    subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + stem + ".fatbin", "--output=" + stem + ".co"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-s", stem + ".co"], check=True, capture_output=True, text=True,
                          timeout=120).stdout
    return set(re.findall(r"\s(\S+)\.kd$", syms, flags=re.M))


def run_units(exe, tmp_path, luts, masks, frames, car, fw, fh, bw, bh, blend=False, fracs=None, env=None):
    """luts: [(int16 [bh,bw,2], uint16 [bh,bw])], masks: [uint8 [bh,bw]], frames: uint8 [n, ncams, fh, fw, 3];
    fracs: [uint32 [bh,bw,2]] 21-bit fractions -> a wide plan (the analytic projection mode); env: the emulator's environment"""
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", fw, fh, bw, bh, len(luts), frames.shape[0], int(car is not None), int(blend) | (2 if fracs is not None else 0)))
        for i, ((m1, m2), mk) in enumerate(zip(luts, masks)):
            f.write(np.ascontiguousarray(m1, np.int16).tobytes())
            f.write(np.ascontiguousarray(m2, np.uint16).tobytes())
            f.write(np.ascontiguousarray(mk, np.uint8).tobytes())
            if fracs is not None:
                f.write(np.ascontiguousarray(fracs[i], np.uint32).tobytes())
        f.write(np.ascontiguousarray(frames, np.uint8).tobytes())
        if car is not None:
            f.write(np.ascontiguousarray(car, np.uint8).tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    nunits, claimed, lines, sectors = struct.unpack("<4i", raw[:16])
    written = np.frombuffer(raw, np.uint8, bw * bh, 16).reshape(bh, bw)
    img = np.frombuffer(raw, np.uint8, frames.shape[0] * bh * bw * 3, 16 + bw * bh).reshape(frames.shape[0], bh, bw, 3)
    return dict(units=nunits, claimed=claimed, lines=lines, sectors=sectors, written=written, img=img, log=r.stdout)


def mask2d(m):
    return m[..., 0] if m.ndim == 3 else m
