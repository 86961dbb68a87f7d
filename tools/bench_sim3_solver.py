#!/usr/bin/env python3
"""Timing of Sim3Solver on MI355X (morb_sim3_solver_batch): batches of 64 problems x ~400 correspondences at 30 % and 60 % outliers on
the device (find(): one call with the whole budget, minInliers 20, device time between events, inputs resident), one problem host to
host (upload, solve, download), and the CPU oracle (tests/native/sim3_solver_oracle.cc, one thread) on the same batches.  Prints one
JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import sim3_solver_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import libc_rand, make_sim3_solver_problem, pack_sim3_solver_problems


def main(reps=20):
    opt = Optimizer(0)
    sim3_solver_oracle.lib()   # compiled before any timing
    res = {}

    def solve(t, its=300):
        return opt.Sim3Solver(t["params"], t["entry"], t["Xw1"], t["Xw2"], t["sigma2_1"], t["sigma2_2"], t["rand"], t["state"], its)

    for of in (0.3, 0.6):
        probs = [make_sim3_solver_problem(480, seed=s, cam1="kb8" if s % 8 == 0 else "pinhole", fix_scale=s % 4 == 0, outlier_frac=of)
                 for s in range(64)]
        rands = [libc_rand(s + 1, 900) for s in range(64)]
        t = pack_sim3_solver_problems(probs, "cuda:0", rand=rands)
        solve(t)
        torch.cuda.synchronize()
        st = Optimizer.sim3_solver_state(t["state"])
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        batch = []
        for _ in range(reps):
            t["state"].zero_()
            ev0.record()
            solve(t)
            ev1.record()
            torch.cuda.synchronize()
            batch.append(ev0.elapsed_time(ev1))
        tag = f"out{int(of * 100)}"
        t0 = time.perf_counter()
        for p, r in zip(probs, rands):
            sim3_solver_oracle.run(p, r)
        res[tag] = dict(correspondences_mean=float(st["N"].mean()), converged=int(st["converged"].sum()),
                        iterations_mean=float(st["iterations"].mean()), batch_ms_median=float(np.median(batch)),
                        batch_ms_min=float(np.min(batch)), oracle_batch_ms=(time.perf_counter() - t0) * 1e3)
    single = []
    for r in range(reps):
        p = make_sim3_solver_problem(480, seed=r, outlier_frac=0.3)
        rnd = [libc_rand(r + 1, 900)]
        t0 = time.perf_counter()
        one = pack_sim3_solver_problems([p], "cuda:0", rand=rnd)
        st, mask, _ = solve(one)
        st.cpu(); mask.cpu()
        single.append((time.perf_counter() - t0) * 1e3)
    res["single_host_to_host_ms_median"] = float(np.median(single))
    p, rnd = make_sim3_solver_problem(480, seed=0, outlier_frac=0.3), libc_rand(1, 900)
    t0 = time.perf_counter()
    sim3_solver_oracle.run(p, rnd)
    res["oracle_single_ms"] = (time.perf_counter() - t0) * 1e3
    res["problems"] = 64
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
