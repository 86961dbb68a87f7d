"""ctypes front of tests/native/essential_graph_oracle.cc, the CPU oracle of Optimizer::OptimizeEssentialGraph on the flattened graph:
compiled into a temporary directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the tests that
rounding and summation order do not move a case's Levenberg-Marquardt path)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "essential_graph_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DEG_ORACLE_REVERSE")   # the second build: fused multiply-adds, edges summed in reverse
# further builds, for the corpus selection only: acos / log one ulp off, or the matrix entries a few ulp off before the factorisation — what
# another libm and another elimination schedule do.  A case that moves under one of them turns on rounding and is no test of a kernel.
PERTURBED_FLAGS = (("-O2", "-ffp-contract=off", "-DEG_ORACLE_NUDGE"), ("-O2", "-ffp-contract=off", "-DEG_ORACLE_JITTER=0"),
                   ("-O2", "-ffp-contract=off", "-DEG_ORACLE_JITTER=3"), ("-O3", "-ffp-contract=fast", "-DEG_ORACLE_NUDGE", "-DEG_ORACLE_JITTER=5"))
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="essential_graph_oracle_"), "libessential_graph_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.eg_oracle_exp.argtypes = [vp, vp]; L.eg_oracle_exp.restype = None
        L.eg_oracle_log.argtypes = [vp, vp]; L.eg_oracle_log.restype = i
        L.eg_oracle_mul.argtypes = [vp, vp, vp]; L.eg_oracle_mul.restype = None
        L.eg_oracle_inverse.argtypes = [vp, vp]; L.eg_oracle_inverse.restype = None
        L.eg_oracle_branches.argtypes = [i, vp, i, vp, vp, vp]; L.eg_oracle_branches.restype = i
        L.eg_oracle_system.argtypes = [i, vp, vp, i, vp, vp, vp, vp, vp]; L.eg_oracle_system.restype = i
        L.eg_oracle_run.argtypes = [i, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp]; L.eg_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def exp(u, flags=DEFAULT_FLAGS):
    u, out = np.ascontiguousarray(u, np.float64), np.zeros(8)
    lib(flags).eg_oracle_exp(_p(u), _p(out))
    return out


def log(S, flags=DEFAULT_FLAGS):
    """(log(S), branch): branch bit 0 = |sigma| < eps, bit 1 = d > 1 - eps."""
    S, out = np.ascontiguousarray(S, np.float64), np.zeros(7)
    br = lib(flags).eg_oracle_log(_p(S), _p(out))
    return out, br


def mul(a, b):
    a, b, out = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64), np.zeros(8)
    lib().eg_oracle_mul(_p(a), _p(b), _p(out))
    return out


def inverse(a):
    a, out = np.ascontiguousarray(a, np.float64), np.zeros(8)
    lib().eg_oracle_inverse(_p(a), _p(out))
    return out


def _arrays(prob):
    return (np.ascontiguousarray(prob["kfSim3"], np.float64).reshape(-1, 8).copy(), np.ascontiguousarray(prob["kfFlags"], np.uint8),
            np.ascontiguousarray(prob["eI"], np.int32), np.ascontiguousarray(prob["eJ"], np.int32),
            np.ascontiguousarray(prob["eSji"], np.float64).reshape(-1, 8))


def branches(prob, S=None):
    """Branches of Sim3::log the edges' errors take at the estimates S (default: the problem's): bit 0 |sigma| < eps, bit 1 d > 1 - eps, bit 2 neither."""
    S0, fl, eI, eJ, M = _arrays(prob)
    S0 = S0 if S is None else np.ascontiguousarray(S, np.float64)
    return lib().eg_oracle_branches(len(S0), _p(S0), len(eI), _p(eI), _p(eJ), _p(M))


def system(prob):
    """The quadratic form at the problem's estimates: (n, H [7n, 7n], b [7n])."""
    S, fl, eI, eJ, M = _arrays(prob)
    n = lib().eg_oracle_system(len(S), _p(S), _p(fl), len(eI), _p(eI), _p(eJ), _p(M), None, None)
    H, b = np.zeros((7 * n, 7 * n)), np.zeros(7 * n)
    lib().eg_oracle_system(len(S), _p(S), _p(fl), len(eI), _p(eI), _p(eJ), _p(M), _p(H), _p(b))
    return n, H, b


def run(prob, flags=DEFAULT_FLAGS):
    """One problem of synth.make_essential_graph_problem.  Returns a dict: kfSim3, mpPos, stats4, chi2."""
    S, fl, eI, eJ, M = _arrays(prob)
    mp = np.ascontiguousarray(prob["mpPos"], np.float32).reshape(-1, 3).copy()
    ref = np.ascontiguousarray(prob["mpRef"], np.int32)
    stats, chi2 = np.zeros(4, np.int32), np.zeros(2)
    lib(flags).eg_oracle_run(len(S), _p(S), _p(fl), len(eI), _p(eI), _p(eJ), _p(M), len(mp), _p(mp), _p(ref), _p(stats), _p(chi2))
    return dict(kfSim3=S, mpPos=mp, stats4=stats, chi2=chi2)
