#!/usr/bin/env python3
"""Timing of Optimizer::InertialOptimization on MI355X (morb_inertial_optimization_batch): one problem of 10, 50 and 200 keyframes and a batch
of 64 problems of 20 keyframes, in each of the three modes; device time between events per call, inputs resident and restored before every
call (the call works in place), beside the CPU oracle (tests/native/inertial_optimization_oracle.cc, dense system, one thread) on the same
problems in the same run.  Also the LM / GN work each call did (outer iterations, trials), so that a time can be read per solve.  Prints one
JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import inertial_optimization_cases as cases
import inertial_optimization_oracle as io
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import make_inertial_optimization_problem, pack_inertial_optimization_problems


def scenes(n, count, mode):
    out = []
    for s in range(count):
        if mode == 1:
            p = make_inertial_optimization_problem(n_kf=n, seed=s, mono=False, s_true=1.0, rwg_deg=0.0, n_imu=20)
            pre = cases.preintegrate(p)
        elif mode == 2:
            p, pre = cases.mode2_scene(n, seed=s)
        else:
            p = make_inertial_optimization_problem(n_kf=n, seed=s, mono=True, s_true=1.2, n_imu=20)
            pre = cases.preintegrate(p)
        out.append((p, pre))
    return out


def main(reps=30):
    opt = Optimizer(0)
    io.lib()   # compiled before any timing
    dev = torch.device("cuda", 0)
    res = {}
    for label, n, count in (("one_problem_10kf", 10, 1), ("one_problem_50kf", 50, 1), ("one_problem_200kf", 200, 1), ("batch64_20kf", 20, 64)):
        for mode in (0, 1, 2):
            sc = scenes(n, count, mode)
            ks, st, hl, pre, fl, pr, g16 = pack_inertial_optimization_problems([p for p, _ in sc], [q for _, q in sc], dev)
            st0, g0 = st.clone(), g16.clone()
            out = None

            def call():
                nonlocal out
                out = opt.InertialOptimization(ks, st, hl, pre, mode, fl, pr, g16, cap=n, out=out)
            for _ in range(3):
                st.copy_(st0); g16.copy_(g0)
                call()
            torch.cuda.synchronize()
            stats = out[1].cpu().numpy()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(reps):
                st.copy_(st0); g16.copy_(g0)
                torch.cuda.synchronize()
                ev0.record()
                call()
                ev1.record()
                torch.cuda.synchronize()
                ms.append(ev0.elapsed_time(ev1))
            t0 = time.perf_counter()
            ostats = [io.run(p, q, mode)["stats"] for p, q in sc]
            oracle_ms = (time.perf_counter() - t0) * 1e3
            res[f"{label}_mode{mode}"] = dict(call_ms_median=float(np.median(ms)), call_ms_min=float(np.min(ms)), call_ms_max=float(np.max(ms)),
                                              oracle_ms=oracle_ms, iterations_mean=float(stats[:, 0].mean()), trials_mean=float(stats[:, 1].mean()),
                                              same_path_as_oracle=int(sum(a.tolist() == b.tolist() for a, b in zip(stats, ostats))), problems=count)
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
