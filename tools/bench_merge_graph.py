#!/usr/bin/env python3
"""Timing of the second overload of Optimizer::OptimizeEssentialGraph on MI355X (morb_optimize_essential_graph_merge) at a merge of
25 + 25 + 500 keyframes: 25 of the merged map, a window of 25 inside the 500 of the old map, covisibility band 10, three old loop edges,
1000 points.  Per call (host arrays in, host arrays out, warmed up): the wall clock of the synchronous call; beside it the one-thread CPU
oracle (tests/native/merge_graph_oracle.cc) on the same problem, the LM work covered (iterations, trials) and the size of the system.
Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SHAPE = dict(n_fixed=25, n_window=25, n_nonfixed=500, band=10, n_old_loops=3, n_points=1000, seed=5)


def main(reps=5):
    import merge_graph_cases as cases
    import merge_graph_oracle as mo
    from morb_slam_amd import Optimizer
    from morb_slam_amd.synth import make_merge_graph_problem
    mo.lib()                        # compiled before any timing
    opt = Optimizer(0)
    p = make_merge_graph_problem(**SHAPE)
    call = lambda: opt.OptimizeEssentialGraphMerge(p["kfLists"], *[p[k] for k in mo.POSES], p["cI"], p["cJ"], p["mpPos"], p["mpRef"])
    got = call()
    t0 = time.perf_counter()
    want = mo.run(p)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    stats = got["stats4"]
    res = dict(keyframes=len(p["kfLists"]), lists=[int((p["kfLists"] == 1).sum()), int((p["kfLists"] & 2 != 0).sum()), int((p["kfLists"] & 4 != 0).sum())],
               candidates=len(p["cI"]), kept=int(got["cKept"].sum()), points=len(p["mpPos"]), stats4=stats.tolist(), chi2=got["chi2"].tolist(),
               same_path_as_oracle=bool(stats.tolist() == want["stats4"].tolist()),
               worst_pose_difference=float(max(np.abs(cases.pose_diff(got[k], want[k])).max() for k in ("kfTcw", "kfTwc"))),
               worst_point_difference=float(np.abs(got["mpPos"] - want["mpPos"]).max()),
               oracle_ms=oracle_ms, wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
               per_trial_ms=float(np.median(wall)) / max(int(stats[1]), 1))
    print(json.dumps(res), flush=True)
    opt.close()


if __name__ == "__main__":
    main()
