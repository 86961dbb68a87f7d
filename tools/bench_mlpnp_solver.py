#!/usr/bin/env python3
"""Timing of MLPnPsolver on MI355X (morb_mlpnp_solver_batch): batches of 64 relocalisation candidates of ~100 and ~300 correspondences
at 30 % and 60 % outliers with Tracking's parameters (0.99, 10, 300, 6, 0.5, 5.991), one iterate(5, ..) call per candidate (which
runs the whole budget unless Refine() returns first): device time between events per launch, inputs resident, beside the CPU oracle
(tests/native/mlpnp_solver_oracle.cc, one thread) on the same problems.  Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import mlpnp_solver_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import libc_rand, make_mlpnp_problem, pack_mlpnp_problems


def main(reps=20, problems=64):
    opt = Optimizer(0)
    mlpnp_solver_oracle.lib()   # compiled before any timing
    res = {"problems": problems}
    for n in (115, 345):        # ~100 and ~300 kept correspondences after the unmatched and bad ones
        for of in (0.3, 0.6):
            probs = [make_mlpnp_problem(n, seed=s, cam="kb8" if s % 8 == 0 else "pinhole", outlier_frac=of) for s in range(problems)]
            rands = [libc_rand(s + 1, 6 * 305) for s in range(problems)]
            t = pack_mlpnp_problems(probs, "cuda:0", rand=rands)

            def solve():
                return opt.MLPnPsolver(t["params"], t["entry"], t["uv"], t["sigma2"], t["Xw"], t["rand"], t["state"], t["bestInliers"], 5)
            solve()
            torch.cuda.synchronize()
            st = Optimizer.mlpnp_solver_state(t["state"])
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            launch = []
            for _ in range(reps):
                t["state"].zero_()
                ev0.record()
                solve()
                ev1.record()
                torch.cuda.synchronize()
                launch.append(ev0.elapsed_time(ev1))
            t0 = time.perf_counter()
            for p, r in zip(probs, rands):
                mlpnp_solver_oracle.run(p, r, calls=[5])
            res[f"n{int(round(float(st['N'].mean()), -1))}_out{int(of * 100)}"] = dict(
                correspondences_mean=float(st["N"].mean()), with_pose=int(st["ok"].sum()), refined=int(st["refined"].sum()),
                iterations_mean=float(st["iterations"].mean()), launch_ms_median=float(np.median(launch)), launch_ms_min=float(np.min(launch)),
                oracle_ms=(time.perf_counter() - t0) * 1e3)
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
