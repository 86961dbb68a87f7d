"""The Python binding is read from include/morb_hip.h (morb_slam_amd/cdecl.py): every prototype gets its ctypes signature, every record
its numpy dtype, and no hand-written copy of either remains in the package.  The reader is checked against an independent regex for
coverage, against the C++ compiler for the layouts, and against small hand-read headers for the type mapping and its refusals."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from morb_slam_amd import cdecl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "morb_slam_amd")
RECORDS = ("morb_keypoint", "morb_frame_params", "morb_sim3_solver_params", "morb_sim3_solver_state", "morb_mlpnp_solver_params",
           "morb_mlpnp_solver_state", "morb_imu_preintegrated")


@pytest.fixture(scope="module")
def header():
    return cdecl.parse(open(os.path.join(INCLUDE, "morb_hip.h"), encoding="utf-8").read(), structures=("morb_frame_params",))


def test_every_declared_function_has_a_parsed_prototype_and_nothing_else(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "morb_hip.h"), encoding="utf-8").read(), flags=re.S)
    names = set(re.findall(r"\b(morb_[a-z0-9_]+)\s*\(", text))
    assert len(names) >= 90
    assert set(header.prototypes) == names
    assert tuple(header.records) == RECORDS
    assert header.constants == {"MORB_OK": 0, "MORB_ERR_INVALID": -1, "MORB_ERR_HIP": -2, "MORB_ERR_CAPACITY": -3,
                                "MORB_ERR_UNSUPPORTED": -4, "MORB_ERR_EMPTY": -5}


def test_record_layouts_equal_the_compilers(header, tmp_path):
    """sizeof / offsetof of every record and field, printed by a C++ program that includes the header itself."""
    lines, want = ["#include <cstddef>", "#include <cstdio>", '#include "morb_hip.h"', "int main() {"], []
    for name, dt in header.records.items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {dt.itemsize}")
        for field in dt.names:
            lines.append(f'  std::printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            want.append(f"{name}.{field} {dt.fields[field][1]} {dt[field].itemsize}")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cc", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(want) == 7 + sum(len(dt.names) for dt in header.records.values()) and len(want) > 80
    assert got == want
    # the ctypes.Structure callers fill by field name has the same layout
    S, dt = header.structures["morb_frame_params"], header.records["morb_frame_params"]
    assert C.sizeof(S) == dt.itemsize and [n for n, _ in S._fields_] == list(dt.names)
    assert [(getattr(S, n).offset, getattr(S, n).size) for n in dt.names] == [(dt.fields[n][1], dt[n].itemsize) for n in dt.names]


def test_the_package_exposes_the_parsed_records(header):
    from morb_slam_amd import capi, optimizer
    assert capi.KP_DTYPE == header.records["morb_keypoint"] and capi.KP_DTYPE.names == ("x", "y", "size", "angle", "response", "octave", "class_id")
    assert issubclass(capi.FrameParams, C.Structure) and C.sizeof(capi.FrameParams) == header.records["morb_frame_params"].itemsize
    assert (capi.MORB_OK, capi.ERR_INVALID, capi.ERR_HIP, capi.ERR_CAPACITY, capi.ERR_UNSUPPORTED, capi.ERR_EMPTY) == (0, -1, -2, -3, -4, -5)
    for name in ("sim3_solver_params", "sim3_solver_state", "mlpnp_solver_params", "mlpnp_solver_state"):
        assert getattr(optimizer, name.upper()) == header.records["morb_" + name]
    pre = header.records["morb_imu_preintegrated"]
    assert optimizer.PREINT_FLOATS * 4 == pre.itemsize and list(optimizer.PREINT_FIELDS) == list(pre.names)
    flat = np.arange(optimizer.PREINT_FLOATS, dtype=np.float32)
    rec = flat.view(pre)[0]
    for field, (off, n) in optimizer.PREINT_FIELDS.items():
        np.testing.assert_array_equal(np.ravel(rec[field]), flat[off:off + n])
    p = capi.make_frame_params(640, 480, 500.0, 501.0, 320.0, 240.0, 40.0, 0.08, [1.0, 1.2], [1.0, 1.44])
    raw = np.frombuffer(bytes(p), header.records["morb_frame_params"])[0]
    assert (raw["maxX"], raw["fy"], raw["mb"], raw["nlevels"]) == (640.0, 501.0, np.float32(0.08), 2)
    assert list(raw["scaleFactors"][:3]) == [1.0, np.float32(1.2), 0.0] and raw["levelSigma2"][1] == np.float32(1.44)


def test_lib_binds_every_exported_function_as_parsed(header):
    from morb_slam_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("libmorb_hip.so is not built")
    assert C.CDLL(capi.LIB_PATH)   # loads without a GPU; no compute call is made here
    L = capi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()
    exported = sorted(ln.split()[-1] for ln in nm if ln.split() and ln.split()[-1].startswith("morb_"))
    assert len(exported) >= 90
    for name in exported:
        restype, argtypes = header.prototypes[name]
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes) and list(fn.argtypes[:]) == [
            C.POINTER(capi.FrameParams) if t is C.POINTER(header.structures["morb_frame_params"]) else t for t in argtypes], name
        assert fn.restype is restype, name
    # a caller may hand over the structure itself or a reference to it
    PP = L.morb_is_in_frustum_batch.argtypes[1]
    params = capi.FrameParams()
    assert PP.from_param(params) is not None and PP.from_param(C.byref(params)) is not None
    # ... and out-parameters are passed by reference, as arrays, as ptr() values or as None
    for arg in (C.byref(C.c_void_p()), C.byref(C.c_int()), (C.c_int * 4)(), capi.ptr(np.zeros(3)), None):
        C.c_void_p.from_param(arg)


# ---- no second copy of the header in the package ---------------------------------------------------------------
_ASSIGN = re.compile(r"\.\s*(argtypes|restype)\b[^=\n]*=(?!=)")
_ON_ENTRY = re.compile(r"\bmorb_\w+\s*\.\s*(?:argtypes|restype)\b")
_ITEMSIZE = re.compile(r"\bitemsize\s*==\s*\d")


def _hand_written(name, text):
    """Lines of a package module that restate the header: a signature set on a morb_ entry or anywhere outside capi.py's one
    binding loop, or a record size pinned to a literal."""
    bad = []
    assigns = 0
    for no, line in enumerate(text.splitlines(), 1):
        code = line.split("#")[0]
        if _ON_ENTRY.search(code) or _ITEMSIZE.search(code):
            bad.append(f"{name}:{no}: {line.strip()}")
        elif _ASSIGN.search(code):
            assigns += 1
            if name != "capi.py" or assigns > 1:
                bad.append(f"{name}:{no}: {line.strip()}")
    return bad


def test_no_hand_written_signature_or_record_size_remains_in_the_package():
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 10
    bad = [b for p in files for b in _hand_written(os.path.basename(p), open(p, encoding="utf-8").read())]
    assert not bad, "the signatures and layouts come from include/morb_hip.h (morb_slam_amd/cdecl.py):\n" + "\n".join(bad)
    capi = open(os.path.join(PKG, "capi.py"), encoding="utf-8").read()
    assert len(_ASSIGN.findall(capi)) == 1 and "HEADER.prototypes.items()" in capi   # the loop is there, and is the only one


def test_scanner_sees_a_table_line_put_back():
    loop = "for name, (restype, argtypes) in HEADER.prototypes.items():\n    fn = getattr(L, name)\n    fn.restype, fn.argtypes = restype, argtypes\n"
    assert _hand_written("capi.py", loop) == []
    assert len(_hand_written("capi.py", loop + "L.morb_extractor_levels.argtypes = [vp]\n")) == 1
    assert len(_hand_written("capi.py", loop + "L.morb_matcher_stream.restype = vp  # handle\n")) == 1
    assert len(_hand_written("optimizer.py", "self._L.morb_ba_schur_profile.argtypes = [C.c_void_p, C.c_int]\n")) == 1
    assert len(_hand_written("optimizer.py", "f = L.morb_ba_solve\nf.argtypes = [vp, vp]\n")) == 1
    assert len(_hand_written("capi.py", loop + "fn.argtypes = argtypes\n")) == 1
    assert len(_hand_written("optimizer.py", "assert SIM3_SOLVER_PARAMS.itemsize == 192 and SIM3_SOLVER_STATE.itemsize == 212\n")) == 1
    assert _hand_written("optimizer.py", "if fn.argtypes == want and rec.itemsize == other.itemsize:  # L.morb_x.argtypes = y\n") == []


# ---- the reader on hand-read headers -----------------------------------------------------------------------------
_SMALL = """
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MORB_OK 0
#define MORB_ERR_EMPTY (-5)   /* empty image */
#define OTHER_THING "text"
typedef struct morb_thing morb_thing;   /* forward */
typedef struct morb_pt {
  float x, y;      /* two per declaration; a ; in a comment */
  int32_t level;
  double w;        /* aligned to 8: four bytes of padding before it */
  float m[3];
} morb_pt;
typedef struct { int n; float v[2], s; } morb_anon;
const char* morb_name(void);
void morb_free(morb_thing*);
int morb_make(morb_thing** out /* , not a parameter */, int n, float f, double d,
              size_t bytes, const uint8_t* image,
              const morb_pt* p, morb_anon*, const unsigned char* flag, void* stream, int32_t q);
void* morb_stream(const morb_thing* t);
size_t morb_bytes(int, int);
float morb_scale(const morb_thing*);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_on_a_small_header():
    h = cdecl.parse(_SMALL, structures=("morb_pt",))
    vp, i = C.c_void_p, C.c_int
    P = C.POINTER(h.structures["morb_pt"])
    assert h.prototypes == {"morb_name": (C.c_char_p, []), "morb_free": (None, [vp]),
                            "morb_make": (i, [vp, i, C.c_float, C.c_double, C.c_size_t, vp, P, vp, vp, vp, i]),
                            "morb_stream": (vp, [vp]), "morb_bytes": (C.c_size_t, [i, i]), "morb_scale": (C.c_float, [vp])}
    assert h.constants == {"MORB_OK": 0, "MORB_ERR_EMPTY": -5}
    pt = h.records["morb_pt"]
    assert pt.names == ("x", "y", "level", "w", "m") and [pt.fields[n][1] for n in pt.names] == [0, 4, 8, 16, 24] and pt.itemsize == 40
    assert pt["m"].shape == (3,) and pt["w"] == np.float64 and pt["level"] == np.int32
    an = h.records["morb_anon"]
    assert an.names == ("n", "v", "s") and [an.fields[n][1] for n in an.names] == [0, 4, 12] and an.itemsize == 16
    assert C.sizeof(h.structures["morb_pt"]) == 40 and h.structures["morb_pt"].w.offset == 16
    assert cdecl.parse(_SMALL).prototypes["morb_make"][1][6] is vp   # no Structure asked for: a plain pointer


@pytest.mark.parametrize("decl, named", [
    ("int morb_f(morb_thing*, long n);", "long"),                          # a scalar type outside the mapping
    ("int morb_f(morb_other* p);", "morb_other"),                          # pointer to a type nobody declared
    ("int morb_f(morb_pt p);", "morb_pt"),                                 # a record by value
    ("int morb_f(int (*cb)(int));", "morb_f"),                             # function pointer
    ("int morb_f();", "morb_f"),                                           # unspecified parameters
    ("short morb_f(void);", "short"),
    ("typedef struct morb_r { char name[8]; } morb_r;", "name[8]"),
    ("typedef struct morb_r { float* p; } morb_r;", "float* p"),
    ("typedef struct morb_r { float m[3][3]; } morb_r;", "m[3][3]"),
    ("typedef int morb_int;", "morb_int"),
    ("extern int morb_counter;", "morb_counter"),
    ("int morb_f(void); int morb_f(void);", "morb_f"),
    ("#define MORB_LIMIT (1 << 4)", "MORB_LIMIT"),
    ("#if 0\nint morb_f(void);\n#endif", "#if 0"),
    ("int morb_f(void)", "morb_f"),                                        # no terminating ;
])
def test_reader_refuses_what_it_does_not_understand(decl, named):
    good = "typedef struct morb_thing morb_thing;\ntypedef struct morb_pt { float x; } morb_pt;\n"
    assert cdecl.parse(good + "int morb_ok(morb_thing*, const morb_pt*);\n").prototypes["morb_ok"] == (C.c_int, [C.c_void_p, C.c_void_p])
    with pytest.raises(ValueError) as e:
        cdecl.parse(good + decl + "\n")
    assert named in str(e.value), str(e.value)


def test_developer_switch_table_lists_exactly_what_the_library_reads():
    """INTEGRATION.md's "Developer switches" table against the getenv("MORB_...") calls of the library's sources: neither may name a
    variable the other does not (rows whose "read by" column is a file under tests/ belong to a test helper, not to the library)."""
    read = set()
    for d in (os.path.join(PKG, "csrc"), INCLUDE):
        for path in glob.glob(os.path.join(d, "**", "*"), recursive=True):
            if os.path.isfile(path):
                read |= set(re.findall(r'getenv\(\s*"(MORB_\w+)"', open(path, encoding="utf-8", errors="replace").read()))
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    table = text[text.index("### Developer switches"):].split("\n## ")[0]
    listed = set()
    for row in re.findall(r"^\|(.+)\|\s*$", table, re.M)[2:]:   # (without the header and its rule)
        variable, read_by = re.split(r"(?<!\\)\|", row)[:2]
        if "tests/" not in read_by:
            listed |= set(re.findall(r"MORB_\w+", variable))
    assert read and read == listed
