"""ctypes front of tests/native/sim3_oracle.cc, the CPU oracle of Optimizer::OptimizeSim3: compiled into a temporary directory
with g++ -O2 -ffp-contract=off on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "sim3_oracle.cc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="sim3_oracle_"), "libsim3_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, SRC])
        L = C.CDLL(out)
        vp = C.c_void_p
        L.sim3_oracle_solve.argtypes = [C.c_int] + [vp] * 12 + [C.c_float, C.c_int, C.c_int, vp, vp, vp]
        L.sim3_oracle_solve.restype = C.c_int
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def solve(prob, bAllPoints=True):
    """One problem of morb_slam_amd.synth.make_sim3_problem -> (nIn, keep u8 [n], S12 f64 [8], stats i32 [8])."""
    n = int(prob["n"])
    a = {k: np.ascontiguousarray(prob[k]) for k in ("entry", "Xw1", "Xw2", "i2", "obs1", "inv1", "obs2", "inv2", "T1w", "T2w", "cam1", "cam2")}
    S = np.array(prob["S12"], np.float64).copy()
    keep = np.zeros(max(n, 1), np.uint8)
    stats = np.zeros(8, np.int32)
    nIn = lib().sim3_oracle_solve(n, *[_p(a[k]) for k in ("entry", "Xw1", "Xw2", "i2", "obs1", "inv1", "obs2", "inv2", "T1w", "T2w", "cam1",
                                                          "cam2")], float(prob["th2"]), int(bool(prob["fix_scale"])), int(bool(bAllPoints)),
                                  _p(S), _p(keep), _p(stats))
    return nIn, keep[:n], S, stats
