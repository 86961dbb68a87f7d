"""Every HIP resource of libmorb_hip.so has one owner: device and pinned memory, streams and events are allocated and released only
inside csrc/hip_owned.h (move-only owners and the one grow-only buffer).  A call anywhere else in csrc/ would bring back a hand-written
release list or a second growth policy.  The C++ adapters above the library keep the same rule for memory: include/morb/ allocates
and frees device and pinned memory only inside device_buffer.h (the per-thread staging every adapter call goes through)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")
OWNER = "hip_owned.h"
ADAPTERS = os.path.join(ROOT, "include", "morb")
ADAPTER_OWNER = "device_buffer.h"

_CALL = re.compile(r"\b(hipMalloc\w*|hipExtMalloc\w*|hipHostMalloc\w*|hipFree\w*|hipHostFree\w*|hipStreamCreate\w*|hipStreamDestroy\w*"
                   r"|hipEventCreate\w*|hipEventDestroy\w*)\s*\(")
# comments and string / character literals, in one pass so that a quote inside a comment (or // inside a string) is read right
_NOISE = re.compile(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", re.S)


def _code(path):
    text = open(path, encoding="utf-8").read()
    return _NOISE.sub(lambda m: "\n" * m.group(0).count("\n") if m.group(0).startswith("/") else '""', text)


def _calls(path):
    code = _code(path)
    return [(code.count("\n", 0, m.start()) + 1, m.group(1)) for m in _CALL.finditer(code)]


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_hip_resources_are_allocated_only_by_the_owner_module():
    bad = [f"{os.path.basename(p)}:{line}: {name}" for p in _sources() if os.path.basename(p) != OWNER for line, name in _calls(p)]
    assert not bad, "allocate / release HIP resources through csrc/hip_owned.h:\n" + "\n".join(bad)


def test_owner_module_is_where_the_calls_are():
    names = {name for _, name in _calls(os.path.join(CSRC, OWNER))}
    for want in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamCreateWithFlags", "hipStreamDestroy",
                 "hipEventCreateWithFlags", "hipEventDestroy"):
        assert want in names, want


def test_adapters_allocate_memory_only_in_the_staging_header():
    mem = re.compile(r"hip(Ext|Host)?(Malloc|Free)\w*")
    headers = sorted(glob.glob(os.path.join(ADAPTERS, "*.h")))
    assert os.path.join(ADAPTERS, ADAPTER_OWNER) in headers
    bad = [f"{os.path.basename(p)}:{line}: {name}" for p in headers if os.path.basename(p) != ADAPTER_OWNER for line, name in _calls(p)
           if mem.fullmatch(name)]
    assert not bad, "stage adapter calls through include/morb/device_buffer.h:\n" + "\n".join(bad)
    names = {name for _, name in _calls(os.path.join(ADAPTERS, ADAPTER_OWNER))}
    for want in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"):
        assert want in names, want


def test_scanner_sees_calls_and_skips_comments_and_strings(tmp_path):
    src = tmp_path / "x.hip"
    src.write_text('// hipMalloc(&p, 1)\n/* hipFree(p);\n */ set_error("hipHostFree(p)");\n'
                   "MORB_HIP_CHECK(hipMalloc (&p, n)); char c = '\"'; hipEventDestroy(e);\n")
    assert _calls(str(src)) == [(4, "hipMalloc"), (4, "hipEventDestroy")]


def _second_argument(code, start):
    """The second argument of the call whose '(' is at code[start]."""
    depth, args, cur = 0, [], []
    for ch in code[start:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                break
        if ch == "," and depth == 1:
            args.append("".join(cur)); cur = []
        else:
            cur.append(ch)
    args.append("".join(cur))
    return args[1] if len(args) > 1 else ""


def _numbered_selectors(path):
    """Workspaces and constant tables of a handle picked by a bare integer: an accessor call whose selector holds a literal, or a
    literal index into a handle's array of them."""
    code = _code(path)
    bad = []
    for m in re.finditer(r"\bmorb_(?:matcher|optimizer)_(?:workspace|const|spill|staging)\s*\(", code):
        if re.search(r"(?<![\w.])\d+\b", _second_argument(code, m.end() - 1)):
            bad.append((code.count("\n", 0, m.start()) + 1, m.group(0).rstrip("( ")))
    for m in re.finditer(r"(?:->|\.)\s*(?:ws|consts)\s*\[\s*[^\]]*?(?<![\w.])\d+\b[^\]]*\]", code):
        bad.append((code.count("\n", 0, m.start()) + 1, m.group(0)))
    return bad


def test_handle_workspaces_are_named_and_the_handles_have_one_definition():
    """A handle's device scratch is a named, typed member of the struct in csrc/handles.h, reached through grow(): no call picks a
    workspace or a constant table by number, and no unit declares the handle structs for itself (which is what made numbered C
    accessors necessary)."""
    bad = [f"{os.path.basename(p)}:{line}: {what}" for p in _sources() for line, what in _numbered_selectors(p)]
    assert not bad, "name the workspace / constant table (csrc/handles.h):\n" + "\n".join(bad)
    decl = re.compile(r"\bstruct\s+morb_(matcher|optimizer)\b")
    stray = [f"{os.path.basename(p)}:{_code(p).count(chr(10), 0, m.start()) + 1}" for p in _sources() if os.path.basename(p) != "handles.h"
             for m in decl.finditer(_code(p))]
    assert not stray, "the handle structs are declared in csrc/handles.h only:\n" + "\n".join(stray)
    assert {m.group(1) for m in decl.finditer(_code(os.path.join(CSRC, "handles.h")))} == {"matcher", "optimizer"}


def test_selector_scanner_sees_numbered_calls(tmp_path):
    src = tmp_path / "y.hip"
    src.write_text("rc = morb_matcher_workspace(m, 5, sizeof(Query) * n, &qs);\n"
                   "rc = morb_matcher_const(m, cam8 ? 1 : 0, thr, sizeof thr, &d, st);\n"
                   "rc = morb_matcher_const(m, cam8 ? morb_matcher::kThresholdsKB8 : morb_matcher::kThresholdsPinhole, thr, 96, &d, st);\n"
                   "rc = grow(m->queries, 2 * (size_t)n, &qs);  // morb_matcher_workspace(m, 5, ...)\n"
                   "return m->ws[which].ensure(bytes, out) + o->consts[2].clock + m->consts[table].clock;\n")
    assert [line for line, _ in _numbered_selectors(str(src))] == [1, 2, 5]
