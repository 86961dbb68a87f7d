"""ctypes front of tests/native/merge_inertial_ba_oracle.cc, the CPU oracle of Optimizer::MergeInertialBA (and, with another plan, of
Optimizer::LocalInertialBA): compiled into a temporary directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another
way, for the test that rounding and summation order do not move the corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "native", "merge_inertial_ba_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-ffp-contract=fast", "-DMIB_ORACLE_REVERSE")   # the second build: fused multiply-adds, points and links in reverse order
# the plan: iterations, initial lambda, erase by chi2 alone, FAIL test (Optimizer.cc:3995, :4280, :4287-4310 | :2324-2897)
MERGE_PLAN = dict(iterations=8, lambda0=1e3, erase_chi2_only=True, fail_test=False)
LOCAL_PLAN = dict(iterations=10, lambda0=1.0, erase_chi2_only=False, fail_test=True)
LOCAL_LARGE_PLAN = dict(iterations=4, lambda0=1e-2, erase_chi2_only=False, fail_test=False)
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="merge_inertial_ba_oracle_"), "libmerge_inertial_ba_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        L = C.CDLL(out)
        vp, i = C.c_void_p, C.c_int
        L.mib_oracle_inertial_edge.argtypes = [vp] * 5
        L.mib_oracle_inertial_edge.restype = None
        L.mib_oracle_oplus.argtypes = [vp] * 4
        L.mib_oracle_oplus.restype = None
        L.mib_oracle_vis_edge.argtypes = [vp] * 9
        L.mib_oracle_vis_edge.restype = i
        L.mib_oracle_run.argtypes = [i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, i] + [vp] * 15
        L.mib_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def cam5_of(prob):
    c = prob["cam"]
    return np.array([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"]], np.float32)


def inertial_edge(pre310, s1, s2):
    """Error (9) and Jacobian (9 x 24: pose 1, v1, bg1, ba1, pose 2, v2) of EdgeInertial between two states of 21 doubles."""
    pre, s1, s2 = np.ascontiguousarray(pre310, np.float32), np.ascontiguousarray(s1, np.float64), np.ascontiguousarray(s2, np.float64)
    e, J = np.zeros(9), np.zeros(216)
    lib().mib_oracle_inertial_edge(_p(pre), _p(s1), _p(s2), _p(e), _p(J))
    return e, J.reshape(9, 24)


def oplus(Tbc12, s21, dx15):
    t, s, d = np.ascontiguousarray(Tbc12, np.float32), np.ascontiguousarray(s21, np.float64), np.ascontiguousarray(dx15, np.float64)
    out = np.zeros(21)
    lib().mib_oracle_oplus(_p(t), _p(s), _p(d), _p(out))
    return out


def vis_edge(prob, s21, X, obs3):
    """Rows, error (3), pose Jacobian (3 x 6) and point Jacobian (3 x 3) of one visual edge of the problem's camera on the state s21."""
    rig = prob.get("rig28")
    c5 = None if rig is not None else cam5_of(prob)
    r28 = None if rig is None else np.ascontiguousarray(rig, np.float32)
    t, s = np.ascontiguousarray(prob["Tbc12"], np.float32), np.ascontiguousarray(s21, np.float64)
    X, o = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(obs3, np.float32)
    e, Jp, Jl = np.zeros(3), np.zeros(18), np.zeros(9)
    rows = lib().mib_oracle_vis_edge(_p(c5), _p(r28), _p(t), _p(s), _p(X), _p(o), _p(e), _p(Jp), _p(Jl))
    return rows, e, Jp.reshape(3, 6), Jl.reshape(3, 3)


def run(prob, pre, plan=MERGE_PLAN, flags=DEFAULT_FLAGS, stop_entry=False, local=False):
    """One problem of morb_slam_amd.synth (make_merge_inertial_ba_problem; local=True: make_inertial_ba_problem, with its mpClose, eRight and
    per-link iRobust / iInfoScale — otherwise every link is robust and unscaled).  pre: [nI, 310] preintegration records.  Returns a dict:
    kfState, mpPos, erase, stats3, info4, linkChi0, chiEnd, depthEnd."""
    kf, mp = np.ascontiguousarray(prob["kfState"], np.float32).copy(), np.ascontiguousarray(prob["mpPos"], np.float32).copy()
    kind = np.ascontiguousarray(prob["kfKind"], np.uint8)
    eKF, eMP = np.ascontiguousarray(prob["eKF"], np.int32), np.ascontiguousarray(prob["eMP"], np.int32)
    obs, inv = np.ascontiguousarray(prob["eObs"], np.float32), np.ascontiguousarray(prob["eInvSigma2"], np.float32)
    i1, i2 = np.ascontiguousarray(prob["iKF1"], np.int32), np.ascontiguousarray(prob["iKF2"], np.int32)
    pre = np.ascontiguousarray(pre, np.float32).reshape(-1, 310)
    nE, nI = len(eKF), len(i1)
    rig = prob.get("rig28")
    r28 = None if rig is None else np.ascontiguousarray(rig, np.float32)
    c5 = None if rig is not None else cam5_of(prob)
    if local:
        close = np.ascontiguousarray(prob["mpClose"], np.uint8)
        right = np.ascontiguousarray(prob["eRight"], np.uint8) if rig is not None else None
        rob, scl = np.ascontiguousarray(prob["iRobust"], np.uint8), np.ascontiguousarray(prob["iInfoScale"], np.float32)
    else:
        close, right, rob, scl = None, None, np.ones(max(nI, 1), np.uint8), np.ones(max(nI, 1), np.float32)
    p5 = np.array([plan["iterations"], plan["lambda0"], plan["erase_chi2_only"], plan["fail_test"], stop_entry], np.float64)
    erase, stats, info = np.zeros(nE, np.uint8), np.zeros(3, np.int32), np.zeros(4, np.int32)
    link0, chi, depth = np.zeros(max(nI, 1)), np.zeros(nE), np.zeros(nE)
    t = np.ascontiguousarray(prob["Tbc12"], np.float32)
    lib(flags).mib_oracle_run(len(kf), _p(kf), _p(kind), len(mp), _p(mp), _p(close), nE, _p(eKF), _p(eMP), _p(obs), _p(right), _p(inv), nI, _p(i1),
                              _p(i2), _p(pre), _p(rob), _p(scl), _p(c5), _p(r28), _p(t), _p(p5), _p(erase), _p(stats), _p(info), _p(link0),
                              _p(chi), _p(depth))
    return dict(kfState=kf, mpPos=mp, erase=erase, stats3=stats, info4=info, linkChi0=link0[:nI], chiEnd=chi, depthEnd=depth)
