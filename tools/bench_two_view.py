#!/usr/bin/env python3
"""Timing of TwoViewReconstruction on MI355X (morb_two_view_reconstruction_batch): 1 and 64 problems of about 300 and about 1500
matches (general scenes, 8 % wrong matches, 200 iterations): device time between events per launch, inputs resident, beside the CPU
oracle (tests/native/two_view_oracle.cc, one thread) on the same problems.  Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import two_view_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.optimizer import TWO_VIEW_STATS
from morb_slam_amd.synth import libc_rand, make_two_view_problem, pack_two_view_problems


def main(reps=10):
    opt = Optimizer(0)
    two_view_oracle.lib()   # compiled before any timing
    res = {}
    for nm, n1, n2 in ((300, 1000, 1040), (1500, 2000, 2100)):
        for problems in (1, 64):
            probs = [make_two_view_problem(s, "general", n1=n1, n2=n2, n_matches=nm) for s in range(problems)]
            rands = [libc_rand(s + 1, 1600) for s in range(problems)]
            t = pack_two_view_problems(probs, "cuda:0", rand=rands)

            def solve():
                return opt.TwoViewReconstruction(t["img1"], t["img2"], t["count"], t["kps"], t["matches12"], t["K4"], t["sigma"], t["rand"], 200)
            out = solve()
            torch.cuda.synchronize()
            stats, ok = out["stats"].cpu().numpy(), out["ok"].cpu().numpy()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            launch = []
            for _ in range(reps):
                ev0.record()
                solve()
                ev1.record()
                torch.cuda.synchronize()
                launch.append(ev0.elapsed_time(ev1))
            t0 = time.perf_counter()
            oks = sum(two_view_oracle.run(p, r)["ok"] for p, r in zip(probs, rands))
            res[f"m{nm}_p{problems}"] = dict(matches_mean=float(stats[:, TWO_VIEW_STATS.index("N")].mean()), reconstructed=int(ok.sum()),
                                             oracle_reconstructed=int(oks), launch_ms_median=float(np.median(launch)),
                                             launch_ms_min=float(np.min(launch)), oracle_ms=(time.perf_counter() - t0) * 1e3)
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
