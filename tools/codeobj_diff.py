#!/usr/bin/env python3
"""Is the device code of two builds of libmorb_hip.so the same?  (No GPU needed.)

    python tools/codeobj_diff.py <libA.so> <libB.so>

Unbundles the gfx950 code object of every translation unit of both libraries and compares, per unit, the disassembly
(`llvm-objdump -d --no-show-raw-insn`) and the kernel descriptors (`llvm-readelf --notes`: registers, LDS, scratch, kernel
arguments).  A host-side change must leave both identical for every unit.  Exit status 0: identical, 1: not."""
import difflib
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_codeobj_cpu import LLVM, _code_objects  # noqa: E402  (the unbundling the code-object tests use)


def _tool(name, *args):
    out = subprocess.run([os.path.join(LLVM, name)] + list(args), capture_output=True, text=True, check=True).stdout
    return [ln for ln in out.splitlines() if "file format" not in ln and not ln.startswith("File:")]   # (those lines name the temporary file)


def _views(lib, tmp):
    os.makedirs(tmp)
    return [(_tool("llvm-objdump", "-d", "--no-show-raw-insn", co), _tool("llvm-readelf", "--notes", co)) for co in _code_objects(lib, tmp)]


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _views(argv[1], os.path.join(tmp, "a")), _views(argv[2], os.path.join(tmp, "b"))
    if len(a) != len(b):
        print(f"DIFFERENT: {len(a)} code objects in {argv[1]}, {len(b)} in {argv[2]}")
        return 1
    # one code object per translation unit, in link order (build.py links the sorted csrc/*.hip)
    units = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(ROOT, "morb_slam_amd", "csrc", "*.hip")))]
    units = units if len(units) == len(a) else [f"code object {i}" for i in range(len(a))]
    same = True
    for unit, (disA, kdA), (disB, kdB) in zip(units, a, b):
        nk = sum(ln.strip().startswith(".name:") for ln in kdA)
        verdict = []
        for what, x, y in (("disassembly", disA, disB), ("kernel descriptors", kdA, kdB)):
            verdict.append(f"{what} {'identical' if x == y else 'DIFFERENT'}")
            if x != y:
                same = False
                for ln in list(difflib.unified_diff(x, y, "A", "B", lineterm="", n=1))[:20]:
                    print("    " + ln)
        print(f"{unit:18s} {nk:4d} kernels, {len(disA):7d} lines: " + ", ".join(verdict))
    print("device code identical" if same else "device code DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
