"""ctypes front of tests/native/merge_graph_oracle.cc, the CPU oracle of the second overload of Optimizer::OptimizeEssentialGraph (map
merging) on the flattened input of morb_optimize_essential_graph_merge.  The builds are those of essential_graph_oracle.py, whose source
the oracle includes: DEFAULT_FLAGS, OTHER_FLAGS (fused multiply-adds, edges summed in reverse) and the perturbed builds of the corpus
selection."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from essential_graph_oracle import DEFAULT_FLAGS, OTHER_FLAGS, PERTURBED_FLAGS   # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "merge_graph_oracle.cc")
POSES = ("kfTcw", "kfTwc", "kfTcwBefMerge", "kfTwcBefMerge")
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="merge_graph_oracle_"), "libmerge_graph_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.mg_oracle_prepare.argtypes = [i, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]; L.mg_oracle_prepare.restype = i
        L.mg_oracle_run.argtypes = [i, vp, vp, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp]; L.mg_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arrays(prob):
    return (np.ascontiguousarray(prob["kfLists"], np.uint8), [np.ascontiguousarray(prob[k], np.float32).reshape(-1, 7).copy() for k in POSES],
            np.ascontiguousarray(prob["cI"], np.int32), np.ascontiguousarray(prob["cJ"], np.int32))


def prepare(prob, flags=DEFAULT_FLAGS):
    """The graph the solver gets: dict(cKept, kfSim3, kfFlags, eI, eJ, eSji)."""
    lists, (Tcw, Twc, TcwBef, TwcBef), cI, cJ = _arrays(prob)
    nKF, nC = len(lists), len(cI)
    kept, est, fl = np.zeros(nC, np.uint8), np.zeros((nKF, 8)), np.zeros(nKF, np.uint8)
    eI, eJ, eS = np.zeros(nC, np.int32), np.zeros(nC, np.int32), np.zeros((nC, 8))
    nE = lib(flags).mg_oracle_prepare(nKF, _p(lists), _p(Tcw), _p(TcwBef), nC, _p(cI), _p(cJ), _p(kept), _p(est), _p(fl), _p(eI), _p(eJ), _p(eS))
    return dict(cKept=kept, kfSim3=est, kfFlags=fl, eI=eI[:nE].copy(), eJ=eJ[:nE].copy(), eSji=eS[:nE].copy())


def run(prob, flags=DEFAULT_FLAGS):
    """One problem of synth.make_merge_graph_problem.  Returns a dict: the four pose arrays, mpPos, cKept, stats4, chi2."""
    lists, poses, cI, cJ = _arrays(prob)
    mp = np.ascontiguousarray(prob["mpPos"], np.float32).reshape(-1, 3).copy()
    ref = np.ascontiguousarray(prob["mpRef"], np.int32)
    kept, stats, chi2 = np.zeros(len(cI), np.uint8), np.zeros(4, np.int32), np.zeros(2)
    lib(flags).mg_oracle_run(len(lists), _p(lists), *[_p(a) for a in poses], len(cI), _p(cI), _p(cJ), _p(kept), len(mp), _p(mp), _p(ref), _p(stats), _p(chi2))
    return dict(zip(POSES, poses), mpPos=mp, cKept=kept, stats4=stats, chi2=chi2)
