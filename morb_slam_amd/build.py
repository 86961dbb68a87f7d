"""Build libmorb_hip.so in-tree with hipcc for gfx950 (explicit command, no JIT cache: the .so travels to the
GPU box with the repo snapshot)."""
import glob
import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_DIR)
CSRC = os.path.join(_DIR, "csrc")
OUT = os.path.join(_DIR, "libmorb_hip.so")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               # one rounding convention shared with the oracle: no mul+add contraction (DESIGN.md "FP conventions")
               "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build_hip(force=False, verbose=False, extra_flags=(), out=OUT):
    """One hipcc -c per translation unit (in parallel, objects under csrc/_obj/), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")) + \
        glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "include", "morb", "*.h"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(CSRC, "_obj" + ("_" + "".join(c for c in "".join(extra_flags) if c.isalnum()) if extra_flags else ""))
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if force or _stale(obj, [src] + hdrs):
            cmd = [hipcc] + flags + ["-c", "-o", obj, src]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            return obj, True
        return obj, False

    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 4)) as ex:
        res = list(ex.map(compile_one, srcs))
    objs = [o for o, _ in res]
    if any(c for _, c in res) or not os.path.exists(out) or _stale(out, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def build_test_native(probe=False):
    """tests/native/libqt_host.so (returned); probe=True (build()) also builds tests/native/libdense_probe.so, which its own tests load through
    build_dense_probe() — the host quadtree's tests do not depend on a device compile."""
    nat = os.path.join(ROOT, "tests", "native")
    out = os.path.join(nat, "libqt_host.so")
    src = os.path.join(nat, "qt_host.cc")
    if _stale(out, [src, os.path.join(CSRC, "quadtree.h")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src])
    if probe:
        build_dense_probe()
        build_math_probe()
    return out


PROBE_OUT = os.path.join(ROOT, "tests", "native", "libdense_probe.so")


def build_dense_probe():
    """tests/native/libdense_probe.so: the dense LDL^T solvers and the MFMA Schur product behind thin test-only entry points, compiled with
    the library's own HIPCC_FLAGS so that the headers build exactly as they do in libmorb_hip.so (which gains no export from it)."""
    src = os.path.join(ROOT, "tests", "native", "dense_probe.hip")
    deps = [src] + [os.path.join(CSRC, h) for h in ("dense_ldlt.h", "schur_mfma.h", "ba_host.h", "wave.h")]
    if _stale(PROBE_OUT, deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-o", PROBE_OUT, src])
    return PROBE_OUT


MATH_PROBE_OUT = os.path.join(ROOT, "tests", "native", "libmath_probe.so")


def build_math_probe():
    """tests/native/libmath_probe.so: the scalar, 3 x 3 and wave-level device functions (libm restatements, camera models, SE3 / SO3 / Sim3
    algebra, small dense helpers, row Jacobi, DPP reductions, RANSAC scaffolding) behind thin test-only entry points.  One translation unit
    per header family (optimizer_device.h and sim3_math.h both define R_to_q in an unnamed namespace), each compiled with the library's
    own HIPCC_FLAGS so that the headers build exactly as they do in libmorb_hip.so (which gains no export from it), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    nat = os.path.join(ROOT, "tests", "native")
    srcs = sorted(glob.glob(os.path.join(nat, "math_probe_*.hip")))
    deps = srcs + [os.path.join(nat, "math_probe_common.h")] + glob.glob(os.path.join(CSRC, "*.h")) + \
        glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "include", "morb", "*.h"))
    if not _stale(MATH_PROBE_OUT, deps):
        return MATH_PROBE_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(nat, "_obj_math_probe")
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        subprocess.check_call([hipcc] + flags + ["-c", "-o", obj, src])
        return obj

    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        objs = list(ex.map(compile_one, srcs))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", MATH_PROBE_OUT] + objs)
    return MATH_PROBE_OUT
