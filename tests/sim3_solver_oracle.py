"""ctypes front of tests/native/sim3_solver_oracle.cc, the CPU oracle of Sim3Solver: compiled into a temporary directory with
g++ -O2 -ffp-contract=off on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "sim3_solver_oracle.cc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="sim3s_oracle_"), "libsim3s_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.sim3s_oracle_run.argtypes = [i] + [vp] * 9 + [i, C.c_double, i, i, i, vp, vp, vp, i, vp, vp, vp, vp]
        L.sim3s_oracle_run.restype = i
        L.sim3s_oracle_budget.argtypes = [i, i, C.c_double, i]
        L.sim3s_oracle_budget.restype = i
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def budget(N, min_inliers, probability=0.99, max_iterations=300):
    return lib().sim3s_oracle_budget(N, min_inliers, probability, max_iterations)


def run(prob, rand, calls=None, hyp_cap=None):
    """One problem of morb_slam_amd.synth.make_sim3_solver_problem, driven like the reference: constructor, SetRansacParameters, then
    iterate(calls[k], ...) until a call converges or reports bNoMore (default: one call with max_iterations, i.e. find()).
    rand = the rand() values in draw order.  Returns a list of per-call dicts and the final best record."""
    n = int(prob["n"])
    calls = np.array(calls if calls is not None else [prob["max_iterations"]], np.int32)
    hyp_cap = hyp_cap if hyp_cap is not None else max(prob["max_iterations"], 1)
    a = {k: np.ascontiguousarray(prob[k]) for k in ("entry", "Xw1", "Xw2", "sigma2_1", "sigma2_2", "T1w", "T2w", "cam1", "cam2")}
    rnd = np.ascontiguousarray(rand, np.int32)
    if len(rnd) == 0:
        rnd = np.zeros(1, np.int32)
    hyp = np.full(hyp_cap, -1, np.int32)
    res = np.zeros((len(calls), 8), np.int32)
    sim3 = np.zeros((len(calls), 16), np.float32)
    mask = np.zeros((len(calls), max(n, 1)), np.uint8)
    best = np.zeros(29, np.float32)
    made = lib().sim3s_oracle_run(n, *[_p(a[k]) for k in ("entry", "Xw1", "Xw2", "sigma2_1", "sigma2_2", "T1w", "T2w", "cam1", "cam2")],
                                  int(prob["fix_scale"]), float(prob["probability"]), int(prob["min_inliers"]), int(prob["max_iterations"]),
                                  len(calls), _p(calls), _p(rnd), _p(hyp), hyp_cap, _p(res), _p(sim3), _p(mask), _p(best))
    out = []
    for k in range(made):
        r = res[k]
        out.append(dict(converged=int(r[0]), noMore=int(r[1]), nInliers=int(r[2]), iterations=int(r[3]), bestInliers=int(r[4]),
                        assigned=int(r[5]), N=int(r[6]), budget=int(r[7]), sim3=sim3[k].copy(), mask=mask[k, :n].copy()))
    return out, dict(bestT12=best[:16].copy(), bestR=best[16:25].copy(), bestt=best[25:28].copy(), bestScale=best[28], hyp=hyp)
