#!/usr/bin/env python3
"""Is the device code of two builds of libmorb_hip.so the same?  (No GPU needed.)

    python tools/codeobj_diff.py <libA.so> <libB.so>

Unbundles the gfx950 code object of every translation unit of both libraries and compares, per kernel or function SYMBOL over all units,
the disassembly (`llvm-objdump -d --no-show-raw-insn`, without the address comment and its `<symbol+0x...>` annotation, which depend on
where the function lies) and the kernel descriptors (`llvm-readelf --notes`: registers, LDS, scratch, kernel arguments).  Code that only
moves between units, or a new unit, leaves every symbol identical; so does a host-side change.  Exit status 0: identical, 1: not."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_codeobj_cpu import LLVM, _code_objects  # noqa: E402  (the unbundling the code-object tests use)


def _tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), capture_output=True, text=True, check=True).stdout.splitlines()


def _by_symbol(lines, start, name, out):
    """Adds to out[symbol] the entries of `lines`: from a line matching `start` to the next unindented line, named by `name`."""
    entries, cur, pc = [], None, set()   # pc: scalar registers holding s_getpc_b64's result until the offset of a global is added to them
    for ln in lines:
        pc |= {"s" + n if n else "vcc_lo" for n in re.findall(r"s_getpc_b64 (?:s\[(\d+):|vcc)", ln)}
        m = re.search(r"s_add_u32 (\w+), \1, 0x[0-9a-f]+", ln)
        if m and m.group(1) in pc:
            pc.remove(m.group(1))
            ln = ln[:ln.index("0x")] + "<pc-relative>"
        if re.match(start, ln):
            cur = []
            entries.append(cur)
        elif ln[:1].strip():
            cur = None
        if cur is not None and ln.strip() not in ("", "..."):   # ("...": zero padding behind a function)
            cur.append(re.sub(r"^[0-9a-f]+ |\s*//.*", "", ln))
    for e in entries:
        m = re.search(name, "\n".join(e), re.M)
        if m:
            out.setdefault(m.group(1), []).append(e)


def _views(lib, tmp):
    os.makedirs(tmp)
    dis, kd = {}, {}   # symbol -> its bodies (a symbol of an unnamed namespace may occur in several units)
    for co in _code_objects(lib, tmp):
        _by_symbol(_tool("llvm-objdump", "-d", "--no-show-raw-insn", co), r"[0-9a-f]+ <.+>:$", r"^<(.+)>:$", dis)
        _by_symbol(_tool("llvm-readelf", "--notes", co), r"  - ", r"^    \.name: +(\S+)$", kd)
    return dis, kd


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _views(argv[1], os.path.join(tmp, "a")), _views(argv[2], os.path.join(tmp, "b"))
    bad = 0
    for what, x, y in (("disassembly", a[0], b[0]), ("kernel descriptor", a[1], b[1])):
        for sym in sorted(set(x) | set(y)):
            xs, ys = sorted(x.get(sym, [])), sorted(y.get(sym, []))
            if xs != ys:
                bad += 1
                print(f"{what} " + (f"DIFFERENT ({sum(map(len, xs))} lines against {sum(map(len, ys))})" if xs and ys else
                                    f"only in {argv[2] if ys else argv[1]}") + f": {sym}")
    print(f"{len(a[0])} symbols, {len(a[1])} kernels: " + ("device code identical" if not bad else f"device code DIFFERS in {bad} places"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
