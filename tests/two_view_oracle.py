"""ctypes front of tests/native/two_view_oracle.cc, the CPU oracle of TwoViewReconstruction: compiled into a temporary directory with
g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the tests that rounding does not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "native", "two_view_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
_libs = {}


def stat_names():
    from morb_slam_amd.optimizer import TWO_VIEW_FSTATS, TWO_VIEW_STATS
    return TWO_VIEW_STATS, TWO_VIEW_FSTATS


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="two_view_oracle_"), "libtwo_view_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.two_view_oracle_run.argtypes = [i, i, vp, vp, vp, vp, C.c_float, i] + [vp] * 9
        L.two_view_oracle_run.restype = i
        L.two_view_oracle_null_vector.argtypes = [vp, i, i, vp]
        L.two_view_oracle_svd3.argtypes = [vp] * 4
        L.two_view_oracle_inverse33.argtypes = [vp] * 2
        L.two_view_oracle_sets.argtypes = [i, i, vp, vp]
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def null_vector(A):
    A = np.ascontiguousarray(A, np.float32)
    x = np.zeros(A.shape[1], np.float32)
    lib().two_view_oracle_null_vector(_p(A), A.shape[0], A.shape[1], _p(x))
    return x


def svd3(M):
    M = np.ascontiguousarray(M, np.float32)
    U, w, V = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((3, 3), np.float32)
    lib().two_view_oracle_svd3(_p(M), _p(U), _p(w), _p(V))
    return U, w, V


def sets(N, max_iterations, rand):
    r = np.ascontiguousarray(rand[:8 * max_iterations], np.int32)
    out = np.zeros((max_iterations, 8), np.int32)
    lib().two_view_oracle_sets(N, max_iterations, _p(r), _p(out))
    return out


def run(prob, rand, flags=DEFAULT_FLAGS):
    """One problem of morb_slam_amd.synth.make_two_view_problem through Reconstruct; rand = the rand() values in draw order, eight per
    iteration.  Returns a dict: ok, T21 [12], P3D [n1, 3], triangulated [n1], stats / fstats (arrays, and every entry by its name),
    inliersH / inliersF [N] by match, hyp [2, max_iterations]."""
    n1, n2, it = int(prob["n1"]), int(prob["n2"]), int(prob["max_iterations"])
    S, F = stat_names()
    kp1, kp2 = np.ascontiguousarray(prob["kp1"], np.float32), np.ascontiguousarray(prob["kp2"], np.float32)
    m12, K4 = np.ascontiguousarray(prob["matches12"], np.int32), np.ascontiguousarray(prob["K4"], np.float32)
    rnd = np.zeros(8 * it, np.int32)
    r = np.asarray(rand, np.int32)[:8 * it]
    rnd[:len(r)] = r
    T21, P3D, tri = np.zeros(12, np.float32), np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    stats, fstats = np.zeros(len(S), np.int32), np.zeros(len(F), np.float32)
    inlH, inlF = np.zeros(max(n1, 1), np.uint8), np.zeros(max(n1, 1), np.uint8)
    hyp = np.zeros((2, it), np.float32)
    ok = lib(flags).two_view_oracle_run(n1, n2, _p(kp1), _p(kp2), _p(m12), _p(K4), float(prob["sigma"]), it, _p(rnd), _p(T21), _p(P3D),
                                        _p(tri), _p(stats), _p(fstats), _p(inlH), _p(inlF), _p(hyp))
    N = int(stats[0])
    o = dict(ok=int(ok), T21=T21, P3D=P3D[:n1], triangulated=tri[:n1], stats=stats, fstats=fstats, inliersH=inlH[:N], inliersF=inlF[:N],
             hyp=hyp)
    o.update({k: int(v) for k, v in zip(S, stats)})
    o.update({k: float(v) for k, v in zip(F, fstats)})
    return o
