"""ctypes front of tests/native/mlpnp_solver_oracle.cc, the CPU oracle of MLPnPsolver: compiled into a temporary directory with
g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the test that rounding does not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "mlpnp_solver_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="mlpnp_oracle_"), "libmlpnp_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.mlpnp_oracle_run.argtypes = [i] + [vp] * 5 + [C.c_double, C.c_float, C.c_float, vp, vp, vp, i, vp, i] + [vp] * 6
        L.mlpnp_oracle_run.restype = i
        L.mlpnp_oracle_residual_jac.argtypes = [vp] * 5
        L.mlpnp_oracle_ransac.argtypes = [i, i, i, i, C.c_float, C.c_double, vp]
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ransac(N, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, probability=0.99):
    """SetRansacParameters on N correspondences -> (adjusted minInliers, budget)."""
    out = np.zeros(3, np.int32)
    lib().mlpnp_oracle_ransac(N, min_inliers, max_iterations, min_set, epsilon, probability, _p(out))
    return int(out[0]), int(out[1])


def residual_jac(x, X, f):
    x, X, f = (np.ascontiguousarray(a, np.float64) for a in (x, X, f))
    r, J = np.zeros(2), np.zeros(12)
    lib().mlpnp_oracle_residual_jac(_p(x), _p(X), _p(f), _p(r), _p(J))
    return r, J.reshape(2, 6)


def run(prob, rand, calls=None, hyp_cap=None, stop=True, flags=DEFAULT_FLAGS, refine_current=False):
    """One problem of morb_slam_amd.synth.make_mlpnp_problem, driven like the reference: constructor, SetRansacParameters, then
    iterate(calls[k], ...) call after call (default: one iterate(5)); with stop, until a call returns true or reports bNoMore.
    rand = the rand() values in draw order, min_set per iteration.  Returns the per-call dicts and a summary (N, adjusted minInliers,
    budget, the per-iteration inlier counts)."""
    n = int(prob["n"])
    calls = np.array(calls if calls is not None else [5], np.int32)
    hyp_cap = hyp_cap if hyp_cap is not None else max(prob["max_iterations"], 1)
    a = {k: np.ascontiguousarray(prob[k]) for k in ("entry", "uv", "sigma2", "Xw", "cam")}
    rnd = np.ascontiguousarray(rand, np.int32)
    nrnd = len(rnd)
    if nrnd == 0:
        rnd = np.zeros(1, np.int32)
    ints = np.array([prob["min_inliers"], prob["max_iterations"], prob["min_set"], len(calls), int(stop), int(refine_current)], np.int32)
    hyp = np.full(hyp_cap, -1, np.int32)
    head = np.zeros(3, np.int32)
    res = np.zeros((len(calls), 7), np.int32)
    Tcw = np.zeros((len(calls), 16), np.float32)
    best = np.zeros((len(calls), 16), np.float32)
    mask = np.zeros((len(calls), max(n, 1)), np.uint8)
    bmask = np.zeros((len(calls), max(n, 1)), np.uint8)
    made = lib(flags).mlpnp_oracle_run(n, *[_p(a[k]) for k in ("entry", "uv", "sigma2", "Xw", "cam")], float(prob["probability"]),
                                       float(prob["epsilon"]), float(prob["th2"]), _p(ints), _p(calls), _p(rnd), nrnd, _p(hyp), hyp_cap,
                                       _p(head), _p(res), _p(Tcw), _p(best), _p(mask), _p(bmask))
    out = []
    for k in range(made):
        r = res[k]
        out.append(dict(ok=int(r[0]), noMore=int(r[1]), nInliers=int(r[2]), iterations=int(r[3]), bestInliers=int(r[4]),
                        refined=int(r[5]), returnedAt=int(r[6]), N=int(head[0]), minInliers=int(head[1]), budget=int(head[2]),
                        Tcw=Tcw[k].copy(), bestTcw=best[k].copy(), mask=mask[k, :n].copy(), bestMask=bmask[k, :n].copy()))
    return out, dict(N=int(head[0]), minInliers=int(head[1]), budget=int(head[2]), hyp=hyp)
