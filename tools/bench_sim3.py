#!/usr/bin/env python3
"""Timing of Optimizer::OptimizeSim3 on MI355X (morb_optimize_sim3_batch): a batch of 64 problems x ~400 correspondences on the device
(device time between events, inputs resident), one problem host to host (upload, solve, download), and the CPU oracle
(tests/native/sim3_oracle.cc, one thread) on the same problems.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import sim3_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import make_sim3_problem, pack_sim3_problems


def main(reps=20):
    probs = [make_sim3_problem(450, seed=s, fix_scale=s % 4 == 0, outlier_frac=0.2, noise_px=0.3) for s in range(64)]
    opt = Optimizer(0)
    t = pack_sim3_problems(probs, "cuda:0")
    S0 = t["S12"].clone()

    def solve(tt):
        return opt.OptimizeSim3(tt["entry"], tt["Xw1"], tt["Xw2"], tt["i2"], tt["obs1"], tt["inv1"], tt["obs2"], tt["inv2"], tt["T1w"], tt["T2w"],
                                tt["cam1"], tt["cam2"], tt["th2"], tt["fix"], tt["S12"], bAllPoints=True, count=tt["count"])

    nIn, keep, stats = solve(t)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    batch = []
    for _ in range(reps):
        t["S12"].copy_(S0)
        ev0.record()
        solve(t)
        ev1.record()
        torch.cuda.synchronize()
        batch.append(ev0.elapsed_time(ev1))
    st = stats.cpu().numpy()
    single = []
    for r in range(reps):
        p = probs[r % len(probs)]
        t0 = time.perf_counter()
        one = pack_sim3_problems([p], "cuda:0")
        n1, k1, s1 = solve(one)
        n1.cpu(); k1.cpu(); one["S12"].cpu(); s1.cpu()
        single.append((time.perf_counter() - t0) * 1e3)
    sim3_oracle.lib()
    t0 = time.perf_counter()
    for p in probs:
        sim3_oracle.solve(p)
    oracle_batch = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sim3_oracle.solve(probs[0])
    oracle_single = (time.perf_counter() - t0) * 1e3
    res = dict(problems=len(probs), correspondences_mean=float(st[:, 5].mean()), lm_iters_mean=float((st[:, 0] + st[:, 2]).mean()),
               lm_trials_mean=float((st[:, 1] + st[:, 3]).mean()), batch_ms_median=float(np.median(batch)), batch_ms_min=float(np.min(batch)),
               single_host_to_host_ms_median=float(np.median(single)), oracle_batch_ms=oracle_batch, oracle_single_ms=oracle_single)
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
