"""ctypes front of tests/native/inertial_optimization_oracle.cc, the CPU oracle of Optimizer::InertialOptimization: compiled into a
temporary directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the test that rounding and
summation order do not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "inertial_optimization_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DIO_ORACLE_REVERSE")   # the second build: fused multiply-adds, links summed in reverse order
PREINT_FLOATS = 310
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="inertial_opt_oracle_"), "libinertial_opt_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.io_oracle_edge.argtypes = [vp] * 8
        L.io_oracle_edge.restype = None
        L.io_oracle_run.argtypes = [i, vp, vp, vp, i, i, f, f, vp, vp, vp, vp]
        L.io_oracle_run.restype = i
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edge(pre, s1, s2, v1, v2, g16):
    """Error (9) and Jacobian (9 x 15: velocity 1, velocity 2, gyro bias, acc bias, gravity direction 2, scale 1) of one EdgeInertialGS."""
    pre, s1, s2 = (np.ascontiguousarray(a, np.float32) for a in (pre, s1, s2))
    v1, v2, g16 = (np.ascontiguousarray(a, np.float64) for a in (v1, v2, g16))
    e, J = np.zeros(9), np.zeros(135)
    lib().io_oracle_edge(_p(pre), _p(s1), _p(s2), _p(v1), _p(v2), _p(g16), _p(e), _p(J))
    return e, J.reshape(9, 15)


def run(prob, pre, mode, flags=DEFAULT_FLAGS, global16=None, has_link=None):
    """One problem of morb_slam_amd.synth.make_inertial_optimization_problem with the preintegrations `pre` [n, 310].  Returns a dict:
    kfState [n, 21] f32, global16 [16] f64, reintegrate [n] u8, stats [4] i32, chi2 [2] f64."""
    n = int(prob["kfState"].shape[0])
    st = np.ascontiguousarray(prob["kfState"], np.float32).copy()
    hl = np.ascontiguousarray(prob["hasLink"] if has_link is None else has_link, np.uint8)
    pre = np.ascontiguousarray(pre, np.float32)
    assert pre.shape == (n, PREINT_FLOATS)
    g16 = np.ascontiguousarray(prob["global16"] if global16 is None else global16, np.float64).copy()
    reint = np.zeros(n, np.uint8)
    stats = np.zeros(4, np.int32)
    chi2 = np.zeros(2)
    lib(flags).io_oracle_run(n, _p(st), _p(hl), _p(pre), int(mode), int(prob["flags"]), float(prob["prior2"][0]), float(prob["prior2"][1]),
                             _p(g16), _p(reint), _p(stats), _p(chi2))
    return dict(kfState=st, global16=g16, reintegrate=reint, stats=stats, chi2=chi2)
