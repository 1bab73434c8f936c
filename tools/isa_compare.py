#!/usr/bin/env python3
"""Do two builds of libbevwarp hold the same gfx950 machine code?

    python tools/isa_compare.py <object dir A> <object dir B>      (e.g. csrc/build of two checkouts, or csrc/build and csrc/build_<tag>)

For every translation unit that is compiled and linked (cameracalibration_amd/build.py: LINKED) the gfx950 code object is taken out of
<dir>/<unit>.o and disassembled; the text is cut at the function symbols, addresses are dropped and every <symbol> operand becomes a
placeholder, so a function's stream does not depend on its (mangled) name or on where it lies.  Printed per unit: the number of kernels on
each side, whether the multisets of stream hashes are equal, and whether the multisets of the kernels' (VGPRs, SGPRs, LDS bytes, scratch
bytes, kernarg bytes) of the code-object notes are equal.  For every function both sides hold under one symbol with different streams: both
instruction counts, every opcode whose count differs (A|B) and, for a kernel, its resources on either side; for every other stream without
a partner, the demangled name.  Exit status 1 unless everything is equal.  It compares two builds and nothing else: for a refactor that
must not change what the compiler emits, or that has to say exactly where it does.
"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cameracalibration_amd.build import LINKED  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM_BIN, name)] + list(args), check=True, capture_output=True, text=True, timeout=600).stdout


def code_object(obj, tmp, tag):
    """The gfx950 code object of a unit's object file (as tests/_native_build.kernels_of takes it out)."""
    stem = os.path.join(tmp, tag + "_" + os.path.basename(obj))
    tool("llvm-objcopy", "--dump-section=.hip_fatbin=" + stem + ".fatbin", obj, stem + ".host")
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + stem + ".fatbin", "--output=" + stem + ".co")
    return stem + ".co"


def streams(co):
    """{function symbol: (sha256 of its instructions and their encodings, names and addresses removed; Counter of its opcodes)}"""
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), (hashlib.sha256(), collections.Counter()))
            continue
        line = re.sub(r"<[^<>]+>", "<sym>", re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line)).strip()   # (the comment: address, then encoding)
        if cur is not None and line:
            cur[0].update(" ".join(line.split()).encode() + b"\n")
            cur[1][line.split()[0]] += 1
    return {k: (h.hexdigest(), ops) for k, (h, ops) in out.items()}


def resources(co):
    """{kernel symbol: (VGPRs, SGPRs, LDS bytes, scratch bytes, kernarg bytes)} from the code-object notes."""
    out = {}
    for entry in re.split(r"^  - (?=\.)", tool("llvm-readelf", "--notes", co), flags=re.M)[1:]:
        keys = dict(re.findall(r"^(?:    )?(\.\w+):\s*(\S+)$", entry, flags=re.M))   # (the entry's own keys; those of .args lie deeper)
        if ".symbol" in keys:
            out[re.sub(r"\.kd$", "", keys[".symbol"].strip("'"))] = tuple(int(keys[r]) for r in RESOURCES)
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM_BIN)
    if not filt or not names:
        return list(names)
    return subprocess.run([filt] + list(names), capture_output=True, text=True, timeout=120).stdout.splitlines()


def main(dir_a, dir_b):
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        for unit in LINKED:
            obj = unit.replace(".hip", ".o")
            cos = [code_object(os.path.join(d, obj), tmp, t) for d, t in ((dir_a, "a"), (dir_b, "b"))]
            st, rs = [streams(c) for c in cos], [resources(c) for c in cos]
            kern = [{k: v for k, v in s.items() if k in r} for s, r in zip(st, rs)]
            other = [{k: v for k, v in s.items() if k not in r} for s, r in zip(st, rs)]
            for s, r in zip(st, rs):
                assert r and set(r) <= set(s), "a kernel of the notes has no code: " + ", ".join(sorted(set(r) - set(s))[:3])
            ha, hb = (collections.Counter(h for h, _ in s.values()) for s in st)
            streams_equal = ha == hb
            res_equal = collections.Counter(rs[0].values()) == collections.Counter(rs[1].values())
            print("%-16s kernels %3d | %3d   other functions %d | %d   streams %s   resources (vgpr, sgpr, lds, scratch, kernarg) %s" % (
                unit.replace(".hip", ""), len(kern[0]), len(kern[1]), len(other[0]), len(other[1]),
                "EQUAL" if streams_equal else "DIFFER", "EQUAL" if res_equal else "DIFFER"))
            # a function of the same symbol on both sides whose stream differs: both instruction counts, the opcodes whose counts differ, and
            # for a kernel its resources on either side
            changed = sorted(k for k in set(st[0]) & set(st[1]) if st[0][k][0] != st[1][k][0] and (ha - hb)[st[0][k][0]] > 0)
            for name, d in zip(changed, demangle(changed)):
                oa, ob = st[0][name][1], st[1][name][1]
                print("    differs: %s\n        instructions %d | %d   %s" % (d, sum(oa.values()), sum(ob.values()), "  ".join(
                    "%s %d|%d" % (op, oa[op], ob[op]) for op in sorted(set(oa) | set(ob)) if oa[op] != ob[op]) or "(the same opcode counts)"))
                if name in rs[0] and name in rs[1]:
                    print("        resources %s | %s" % (rs[0][name], rs[1][name]))
            for side, mine, theirs in (("A", st[0], hb), ("B", st[1], ha)):   # one name per copy of a stream the other side lacks
                lack = collections.Counter(h for h, _ in mine.values()) - theirs
                lone = []
                for name, (h, _) in sorted(mine.items()):
                    if lack[h] > 0:
                        lack[h] -= 1
                        if name not in changed:
                            lone.append(name)
                for d in demangle(lone):
                    print("    only in %s: %s" % (side, d))
            same = same and streams_equal and res_equal and len(kern[0]) == len(kern[1])
    print("identical machine code in all %d units" % len(LINKED) if same else "THE BUILDS DIFFER")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
