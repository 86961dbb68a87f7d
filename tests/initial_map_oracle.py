"""ctypes front of tests/native/initial_map_oracle.cc, the CPU oracle of the numeric part of Tracking::CreateInitialMapMonocular: compiled
into a temporary directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the test that rounding and
summation order do not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "initial_map_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DIM_ORACLE_REVERSE")   # the second build: fused multiply-adds, points visited in reverse order
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="initial_map_oracle_"), "libinitial_map_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.im_oracle_edge.argtypes = [i] + [vp] * 7
        L.im_oracle_edge.restype = None
        L.im_oracle_oplus.argtypes = [vp] * 3
        L.im_oracle_oplus.restype = None
        L.im_oracle_run.argtypes = [i, vp, vp, vp, i, i, vp, i, vp, vp, vp, vp, i, vp, i, i, f, i, i] + [vp] * 8
        L.im_oracle_run.restype = i
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edge(kb8, cam8, T12, X, obs):
    """Error (2), pose Jacobian (2 x 6) and point Jacobian (2 x 3) of one EdgeSE3ProjectXYZ; T12 = R (row-major) then t, f64."""
    cam8 = np.ascontiguousarray(cam8, np.float32)
    T12, X, obs = (np.ascontiguousarray(a, np.float64) for a in (T12, X, obs))
    e, Jp, Jl = np.zeros(2), np.zeros(12), np.zeros(6)
    lib().im_oracle_edge(int(kb8), _p(cam8), _p(T12), _p(X), _p(obs), _p(e), _p(Jp), _p(Jl))
    return e, Jp.reshape(2, 6), Jl.reshape(2, 3)


def oplus(T12, u):
    T12, u = np.ascontiguousarray(T12, np.float64), np.ascontiguousarray(u, np.float64)
    out = np.zeros(12)
    lib().im_oracle_oplus(_p(T12), _p(u), _p(out))
    return out


def run(prob, nIterations=20, robust=True, depthScale=1.0, minTracked=50, stop=False, flags=DEFAULT_FLAGS, ok=None):
    """One problem of morb_slam_amd.synth.make_initial_map_problem.  Returns a dict: status, Tcw2 [12], mpPos / mpNormal [n1, 3], mpDist
    [n1, 2], hasMP [n1], stats [4] (points, outer iterations, trials, stop seen), chi2 [2], median."""
    n1, n2 = int(prob["n1"]), int(prob["n2"])
    a = {k: np.ascontiguousarray(prob[k], np.float32) for k in ("cam8", "levelSigma2", "scaleFactors", "kp1", "kp2", "P3D", "T21")}
    ls, sf = np.zeros(16, np.float32), np.zeros(16, np.float32)
    ls[:len(a["levelSigma2"])], sf[:len(a["scaleFactors"])] = a["levelSigma2"], a["scaleFactors"]
    m12, tri = np.ascontiguousarray(prob["matches12"], np.int32), np.ascontiguousarray(prob["triangulated"], np.uint8)
    T, pos, nrm, dist = np.zeros(12, np.float32), np.zeros((n1, 3), np.float32), np.zeros((n1, 3), np.float32), np.zeros((n1, 2), np.float32)
    has, stats, chi2, med = np.zeros(n1, np.uint8), np.zeros(4, np.int32), np.zeros(2), np.zeros(1, np.float32)
    st = lib(flags).im_oracle_run(int(prob["kb8"]), _p(a["cam8"]), _p(ls), _p(sf), int(prob["nlevels"]), n1, _p(a["kp1"]), n2, _p(a["kp2"]), _p(m12),
                                  _p(tri), _p(a["P3D"]), int(prob["ok"] if ok is None else ok), _p(a["T21"]), int(nIterations), int(bool(robust)),
                                  float(depthScale), int(minTracked), int(bool(stop)), _p(T), _p(pos), _p(nrm), _p(dist), _p(has), _p(stats),
                                  _p(chi2), _p(med))
    return dict(status=st, Tcw2=T, mpPos=pos, mpNormal=nrm, mpDist=dist, hasMP=has, stats=stats, chi2=chi2, median=float(med[0]))
