#!/usr/bin/env python3
"""Timing of MergeInertialBA on MI355X (morb_merge_inertial_ba) at the reference's largest graph: 13 keyframes of 15 unknowns, 30 free in
the pose only, one fixed, about 24 k edges (P = 375).  Per call (host arrays in, host arrays out, warmed up): the wall clock of the
synchronous call, median of `reps` calls; beside it the one-thread CPU oracle (tests/native/merge_inertial_ba_oracle.cc) on the same
problem.  `--local LIB`: instead, morb_local_inertial_ba at the 10-keyframe window of make_inertial_ba_problem(n_opt=10, seed=1) through
the library at LIB (any build that exports it: the kernels are shared, so two builds are compared by running this on each, interleaved).
Prints one JSON line; numbers only, no threshold."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def _wall(call, reps, warm=10):
    for _ in range(warm):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms_median=float(np.median(ts)), wall_ms_min=float(np.min(ts)), wall_ms_max=float(np.max(ts)), reps=reps)


def local(lib_path, reps):
    import merge_inertial_ba_cases as cases
    from morb_slam_amd.capi import HEADER
    from morb_slam_amd.synth import make_inertial_ba_problem
    L = C.CDLL(lib_path)
    for name in ("morb_optimizer_create", "morb_optimizer_destroy", "morb_local_inertial_ba"):
        getattr(L, name).restype, getattr(L, name).argtypes = HEADER.prototypes[name]
    p = make_inertial_ba_problem(n_opt=10, seed=1)
    pre = np.ascontiguousarray(cases.preintegrate(p), np.float32)
    h = C.c_void_p()
    assert L.morb_optimizer_create(C.byref(h), 0) == 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    a = [np.ascontiguousarray(p[k], t) for k, t in (("kfKind", np.uint8), ("mpClose", np.uint8), ("eKF", np.int32), ("eMP", np.int32), ("eObs", np.float32),
                                                    ("eInvSigma2", np.float32), ("iKF1", np.int32), ("iKF2", np.int32), ("iRobust", np.uint8),
                                                    ("iInfoScale", np.float32), ("Tbc12", np.float32))]
    erase, stats, c = np.zeros(len(a[2]), np.uint8), np.zeros(3, np.int32), p["cam"]

    def call():
        kf, mp = p["kfState"].copy(), p["mpPos"].copy()
        rc = L.morb_local_inertial_ba(h, len(kf), ptr(kf), ptr(a[0]), len(mp), ptr(mp), ptr(a[1]), len(a[2]), ptr(a[2]), ptr(a[3]), ptr(a[4]), ptr(a[5]),
                                      len(a[6]), ptr(a[6]), ptr(a[7]), ptr(pre), ptr(a[8]), ptr(a[9]), c["fx"], c["fy"], c["cx"], c["cy"], c["bf"],
                                      ptr(a[10]), 0, ptr(erase), ptr(stats))
        assert rc == 0
    r = dict(lib=os.path.basename(lib_path), edges=len(a[2]), points=len(p["mpPos"]), **_wall(call, reps))
    r["stats3"] = stats.tolist()
    L.morb_optimizer_destroy(h)
    return r


def merge(reps):
    import merge_inertial_ba_cases as cases
    import merge_inertial_ba_oracle as mo
    from morb_slam_amd import Optimizer
    from morb_slam_amd.synth import make_merge_inertial_ba_problem
    mo.lib()                        # compiled before any timing
    opt = Optimizer(0)
    res = {}
    for name, kw in (("mix", dict(mono_frac=0.3)), ("kb8", dict(kb8=True))):
        p = make_merge_inertial_ba_problem(n_cur=6, n_merge=6, n_cov=30, n_points=4600, seed=1, **kw)
        pre = cases.preintegrate(p)
        call = lambda: opt.MergeInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"],
                                           pre, p["cam"], p["Tbc12"], rig=p["rig28"])
        out = call()
        t0 = time.perf_counter()
        want = mo.run(p, pre)
        oracle_ms = (time.perf_counter() - t0) * 1e3
        res[name] = dict(free15=int((p["kfKind"] == 0).sum()), free6=int((p["kfKind"] == 3).sum()), unknowns=int(15 * (p["kfKind"] == 0).sum() + 6 * (p["kfKind"] == 3).sum()),
                         points=len(p["mpPos"]), edges=len(p["eKF"]), links=len(p["iKF1"]), stats3=out[3].tolist(),
                         same_path_as_oracle=bool(out[3].tolist() == want["stats3"].tolist() and (out[2] == want["erase"]).all()),
                         oracle_ms=oracle_ms, merge=_wall(call, reps))
    opt.close()
    return res


if __name__ == "__main__":
    reps = 40
    if len(sys.argv) > 2 and sys.argv[1] == "--local":
        print(json.dumps(local(sys.argv[2], reps)))
    else:
        print(json.dumps(merge(reps)))
