"""ctypes front of tests/native/pose_graph_4dof_oracle.cc, the CPU oracle of Optimizer::OptimizeEssentialGraph4DoF on the flattened graph:
compiled into a temporary directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the tests that
rounding and summation order do not move a case's Levenberg-Marquardt path)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "pose_graph_4dof_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DPG4_ORACLE_REVERSE")   # the second build: fused multiply-adds, edges summed in reverse
# further builds, for the corpus selection only (the method of profiles/r17/README.md): acos / sin one ulp off, or the matrix entries a few
# ulp off before the factorisation — what another libm and another elimination schedule do
PERTURBED_FLAGS = (("-O2", "-ffp-contract=off", "-DPG4_ORACLE_NUDGE"), ("-O2", "-ffp-contract=off", "-DPG4_ORACLE_JITTER=0"),
                   ("-O2", "-ffp-contract=off", "-DPG4_ORACLE_JITTER=3"), ("-O3", "-ffp-contract=fast", "-DPG4_ORACLE_NUDGE", "-DPG4_ORACLE_JITTER=5"))
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="pose_graph_4dof_oracle_"), "libpose_graph_4dof_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.pg4_oracle_error.argtypes = [vp, vp, vp, vp]; L.pg4_oracle_error.restype = None
        L.pg4_oracle_oplus.argtypes = [vp, vp, vp, vp]; L.pg4_oracle_oplus.restype = None
        L.pg4_oracle_system.argtypes = [i, vp, vp, vp, vp, i, vp, vp, vp, d, vp, vp, vp, vp, vp]; L.pg4_oracle_system.restype = i
        L.pg4_oracle_run.argtypes = [i, vp, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp, vp, vp]; L.pg4_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def error(Pi, Pj, T, flags=DEFAULT_FLAGS):
    """Edge4DoF::computeError on two camera poses and a measurement (12 doubles each: R row-major, t)."""
    Pi, Pj, T = (np.ascontiguousarray(a, np.float64).reshape(12) for a in (Pi, Pj, T))
    e = np.zeros(6)
    lib(flags).pg4_oracle_error(_p(Pi), _p(Pj), _p(T), _p(e))
    return e


def oplus(body12, Tcb12, u4, flags=DEFAULT_FLAGS):
    """The camera pose of a fresh vertex (DR = I) with body state body12 after VertexPose4DoF::oplusImpl(u4)."""
    body12, u4 = np.ascontiguousarray(body12, np.float64).reshape(12), np.ascontiguousarray(u4, np.float64).reshape(4)
    tcb, out = np.ascontiguousarray(Tcb12, np.float32).reshape(12), np.zeros(12)
    lib(flags).pg4_oracle_oplus(_p(body12), _p(tcb), _p(u4), _p(out))
    return out


def _arrays(prob):
    return (np.ascontiguousarray(prob["kfPose"], np.float64).reshape(-1, 12).copy(), np.ascontiguousarray(prob["kfBody"], np.float64).reshape(-1, 12),
            np.ascontiguousarray(prob["kfFixed"], np.uint8), np.ascontiguousarray(prob["Tcb12"], np.float32).reshape(12),
            np.ascontiguousarray(prob["eI"], np.int32), np.ascontiguousarray(prob["eJ"], np.int32),
            np.ascontiguousarray(prob["eTij"], np.float64).reshape(-1, 12))


def system(prob, lam=0.0, flags=DEFAULT_FLAGS):
    """The quadratic form at the problem's states: (n, H [4n, 4n], b [4n], x [4n] = the envelope solve of (H + lam I) x = b, ok, J [nE, 2, 6, 4])."""
    P, B, fx, tcb, eI, eJ, M = _arrays(prob)
    L = lib(flags)
    n = L.pg4_oracle_system(len(P), _p(P), _p(B), _p(fx), _p(tcb), len(eI), _p(eI), _p(eJ), _p(M), lam, None, None, None, None, None)
    H, b, x, ok, J = np.zeros((4 * n, 4 * n)), np.zeros(4 * n), np.zeros(4 * n), np.zeros(1, np.int32), np.zeros((len(eI), 2, 6, 4))
    L.pg4_oracle_system(len(P), _p(P), _p(B), _p(fx), _p(tcb), len(eI), _p(eI), _p(eJ), _p(M), lam, _p(H), _p(b), _p(x), _p(ok), _p(J))
    return n, H, b, x, bool(ok[0]), J


def run(prob, flags=DEFAULT_FLAGS):
    """One problem of synth.make_pose_graph_4dof_problem.  Returns a dict: kfPose, mpPos, stats4, chi2, accepted (steps)."""
    P, B, fx, tcb, eI, eJ, M = _arrays(prob)
    mp = np.ascontiguousarray(prob["mpPos"], np.float32).reshape(-1, 3).copy()
    ref = np.ascontiguousarray(prob["mpRef"], np.int32)
    scw = np.ascontiguousarray(prob["kfScw"], np.float64).reshape(-1, 8)
    stats, chi2, acc = np.zeros(4, np.int32), np.zeros(2), np.zeros(1, np.int32)
    lib(flags).pg4_oracle_run(len(P), _p(P), _p(B), _p(fx), _p(tcb), len(eI), _p(eI), _p(eJ), _p(M), len(mp), _p(mp), _p(ref), _p(scw), _p(stats), _p(chi2), _p(acc))
    return dict(kfPose=P, mpPos=mp, stats4=stats, chi2=chi2, accepted=int(acc[0]))
