#!/usr/bin/env python3
"""Timing of the welding bundle adjustment of map merging on MI355X (morb_merge_bundle_adjustment) at LoopClosing::MergeLocal's own size:
25 free + 25 fixed keyframes (numTemporalKFs = 25), the points they share, about 25 k edges.  Per call (host arrays in, host arrays out,
warmed up): device time between two events recorded around the synchronised call, and the wall clock of the call; beside it the one-thread
CPU oracle (tests/native/merge_ba_oracle.cc) on the same problem, and morb_local_bundle_adjustment on the same graph as the yardstick for
what one robust round of up to ten iterations costs.  Also the LM work each covers (iterations, trials, slots and launches of the queue).
Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import merge_ba_oracle as mo
from morb_slam_amd import Optimizer
from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
from morb_slam_amd.synth import make_merge_ba_problem


def _time(call, reps):
    for _ in range(3):
        call()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        call()
        ev1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev0.elapsed_time(ev1))
    return dict(event_ms_median=float(np.median(dev)), event_ms_min=float(np.min(dev)), event_ms_max=float(np.max(dev)),
                wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)))


def main(reps=20):
    torch.zeros(1, device="cuda")   # (the events need the device)
    opt = Optimizer(0)
    mo.lib()                        # compiled before any timing
    res = {}
    for name, kw in (("mix", dict(mono_frac=0.3)), ("kb8", dict(kb8=True))):
        p = make_merge_ba_problem(25, 25, 3500, seed=1, **kw)
        args = (p["kfPose"], p["kfFixed"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"])
        out = opt.MergeBundleAdjustment(*args, camL=p["camL"])
        stats = out[4].tolist()
        t0 = time.perf_counter()
        want = mo.run(p)
        oracle_ms = (time.perf_counter() - t0) * 1e3
        slots = stats[1] + 1 + stats[3]          # round-1 trials, the hand-over, round-2 trials
        r = dict(keyframes=len(p["kfPose"]), free_keyframes=int((p["kfFixed"] == 0).sum()), points=len(p["mpPos"]), edges=len(p["eKF"]), stats6=stats,
                 slots=slots, launches=4 + 7 * slots, launches_queued_ahead_at_most=7,
                 same_path_as_oracle=bool(stats == want["stats6"].tolist() and (out[2] == want["erase"]).all() and (out[3] == want["level"]).all()),
                 oracle_ms=oracle_ms, merge=_time(lambda: opt.MergeBundleAdjustment(*args, camL=p["camL"]), reps))
        if name == "mix":
            lba = local_bundle_adjustment_oneshot(opt, *args)
            r["local_ba_same_graph"] = dict(stats2=lba[3].tolist(), launches=3 + 7 * int(lba[3][1]),
                                            **_time(lambda: local_bundle_adjustment_oneshot(opt, *args), reps))
        res[name] = r
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
