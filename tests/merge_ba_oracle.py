"""ctypes front of tests/native/merge_ba_oracle.cc, the CPU oracle of the welding bundle adjustment of map merging
(Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)): compiled into a temporary directory with g++ -O2
-ffp-contract=off on first use (lib(flags) builds it another way, for the test that rounding and summation order do not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "merge_ba_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DMB_ORACLE_REVERSE")   # the second build: fused multiply-adds, points visited in reverse order
MERGE_PLAN = ((5, 1, 5.99), (10, 0, 5.99))        # Optimizer.cc:3547, :3654, :3697: (iterations, robust, monocular delta^2) per round
LOCAL_BA_PLAN = ((10, 1, 5.991),)                 # LocalBundleAdjustment (Optimizer.cc:1053-1441) as one round of this oracle
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="merge_ba_oracle_"), "libmerge_ba_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.mb_oracle_edge.argtypes = [i] + [vp] * 7
        L.mb_oracle_edge.restype = i
        L.mb_oracle_oplus.argtypes = [vp] * 3
        L.mb_oracle_oplus.restype = None
        L.mb_oracle_run.argtypes = [i, vp, i, vp, vp, i, vp, i, vp, vp, vp, vp, i, vp, vp, vp, C.c_double, i, i] + [vp] * 6
        L.mb_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edge(kb8, cam8, T12, X, obs3):
    """Rows, error (3), pose Jacobian (3 x 6) and point Jacobian (3 x 3) of one edge; T12 = R (row-major) then t, f64; obs3[2] < 0: monocular."""
    cam8, obs3 = np.ascontiguousarray(cam8, np.float32), np.ascontiguousarray(obs3, np.float32)
    T12, X = np.ascontiguousarray(T12, np.float64), np.ascontiguousarray(X, np.float64)
    e, Jp, Jl = np.zeros(3), np.zeros(18), np.zeros(9)
    rows = lib().mb_oracle_edge(int(kb8), _p(cam8), _p(T12), _p(X), _p(obs3), _p(e), _p(Jp), _p(Jl))
    return rows, e, Jp.reshape(3, 6), Jl.reshape(3, 3)


def oplus(T12, u):
    T12, u = np.ascontiguousarray(T12, np.float64), np.ascontiguousarray(u, np.float64)
    out = np.zeros(12)
    lib().mb_oracle_oplus(_p(T12), _p(u), _p(out))
    return out


def cam8_of(prob):
    """(kb8, cam8) of a synth problem: its KannalaBrandt8 camera, or fx fy cx cy bf of the pinhole one."""
    if prob.get("camL") is not None:
        return 1, np.ascontiguousarray(prob["camL"], np.float32)
    c = prob["cam"]
    return 0, np.array([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], 0, 0, 0], np.float32)


def run(prob, plan=MERGE_PLAN, flags=DEFAULT_FLAGS, user_lambda=0.0, stop_entry=False, stop_after=0):
    """One problem of morb_slam_amd.synth (make_merge_ba_problem, make_ba_problem).  Returns a dict: kfPose, mpPos, erase, level, stats6,
    chiStale, chiFresh, info4 (round 1 ended on a rejected trial, points / free keyframes that lose all their edges, edges erased on a
    stale chi2 whose fresh chi2 passes)."""
    kb8, cam8 = cam8_of(prob)
    kf, mp = np.ascontiguousarray(prob["kfPose"], np.float32).copy(), np.ascontiguousarray(prob["mpPos"], np.float32).copy()
    fixed = np.ascontiguousarray(prob["kfFixed"], np.uint8)
    eKF, eMP = np.ascontiguousarray(prob["eKF"], np.int32), np.ascontiguousarray(prob["eMP"], np.int32)
    obs = np.ascontiguousarray(prob["eObs"], np.float32)
    if obs.shape[1] == 2:
        obs = np.ascontiguousarray(np.concatenate([obs, -np.ones((len(obs), 1), np.float32)], 1))
    inv = np.ascontiguousarray(prob["eInvSigma2"], np.float32)
    nE = len(eKF)
    its = np.array([r[0] for r in plan], np.int32); rob = np.array([r[1] for r in plan], np.int32); d2 = np.array([r[2] for r in plan], np.float64)
    erase, level, stats, info = np.zeros(nE, np.uint8), np.zeros(nE, np.uint8), np.zeros(6, np.int32), np.zeros(4, np.int32)
    stale, fresh = np.zeros(nE), np.zeros(nE)
    lib(flags).mb_oracle_run(kb8, _p(cam8), len(kf), _p(kf), _p(fixed), len(mp), _p(mp), nE, _p(eKF), _p(eMP), _p(obs), _p(inv), len(plan), _p(its),
                             _p(rob), _p(d2), float(user_lambda), int(bool(stop_entry)), int(stop_after), _p(erase), _p(level), _p(stats), _p(stale),
                             _p(fresh), _p(info))
    return dict(kfPose=kf, mpPos=mp, erase=erase, level=level, stats6=stats, chiStale=stale, chiFresh=fresh, info4=info)
