#!/usr/bin/env python3
"""Timing of the numeric part of Tracking::CreateInitialMapMonocular on MI355X (morb_create_initial_map_monocular_batch): 1, 64 and 512
problems of 150 and of 600 points (pinhole, robust, 20 iterations, the reference's call), device time between events per call with the
inputs resident (the call does not work in place), beside the CPU oracle (tests/native/initial_map_oracle.cc, dense normal equations, one
thread) on the same problems in the same run: the oracle runs the first 16 problems of a batch, its time for the batch is that mean times
the count.  Also the LM work each call did (outer iterations, trials), so that a time can be read per solve.  Prints one JSON line; numbers
only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import initial_map_oracle as io
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import initial_map_frame_params, make_initial_map_problem, pack_initial_map_problems


def main(reps=20):
    opt = Optimizer(0)
    io.lib()   # compiled before any timing
    dev = torch.device("cuda", 0)
    res = {}
    for npts in (150, 600):
        for count in (1, 64, 512):
            probs = [make_initial_map_problem(seed=5000 + s, n_points=npts, noise_px=1.0, point_noise=0.01, pose_noise=(0.003, 0.01)) for s in range(count)]
            t = pack_initial_map_problems(probs, dev)
            P = initial_map_frame_params(probs[0])
            out = None

            def call():
                nonlocal out
                out = opt.CreateInitialMapMonocular(P, t["img1"], t["img2"], t["count"], t["kps"], t["matches12"], t["ok"], t["T21"], t["P3D"],
                                                    t["triangulated"], nIterations=20, robust=True, out=out, stream=torch.cuda.current_stream().cuda_stream)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            stats, status = out["stats"].cpu().numpy(), out["status"].cpu().numpy()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(reps):
                torch.cuda.synchronize()
                ev0.record()
                call()
                ev1.record()
                torch.cuda.synchronize()
                ms.append(ev0.elapsed_time(ev1))
            k = min(count, 16)
            t0 = time.perf_counter()
            ostats = [io.run(p, 20, True)["stats"] for p in probs[:k]]
            oracle_ms = (time.perf_counter() - t0) * 1e3 / k
            res[f"{count}x{npts}pts"] = dict(call_ms_median=float(np.median(ms)), call_ms_min=float(np.min(ms)), call_ms_max=float(np.max(ms)),
                                             oracle_ms_per_problem=oracle_ms, oracle_ms_batch=oracle_ms * count, oracle_problems_run=k,
                                             iterations_mean=float(stats[:, 1].mean()), trials_mean=float(stats[:, 2].mean()),
                                             same_path_as_oracle=int(sum(a.tolist() == b.tolist() for a, b in zip(stats[:k], ostats))),
                                             status_ok=int((status == 1).sum()), problems=count, cap=int(t["matches12"].shape[1]))
    print(json.dumps(res))
    opt.close()


if __name__ == "__main__":
    main()
