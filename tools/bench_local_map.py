#!/usr/bin/env python3
"""Timing of Tracking::UpdateLocalMap on MI355X (morb_update_local_map_batch, and morb_gather_local_map_points_batch behind it): synthetic
maps of 500 and of 2000 keyframes (morb_slam_amd.synth.make_local_map_scene: about 200 points per keyframe, tracks of about ten keyframes,
so that a covisible pair of keyframes shares about 100 points), 1 and 256 frames per call: device time between events per call after
warm-up, the map tables resident, beside the CPU oracle (tests/native/local_map_oracle.cc, one thread; only its two reference functions
are timed, not the building of its objects) on the same frames, under a time limit per step.  Prints one JSON line; numbers only, no
threshold."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import local_map_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.synth import make_local_map_scene


def main(reps=20, sizes=(500, 2000), batches=(1, 256), oracle_limit_s=10.0):
    m = ORBmatcher(0.8, True)
    oracle.lib()   # compiled before any timing
    dev = "cuda:0"
    res = {}
    for nkf in sizes:
        scene = make_local_map_scene(seed=11, nkf=nkf, nmp=18 * nkf, kf_cap=320, nq=max(batches), cap=512, track=10, stray_frac=0.0)
        tables = ORBmatcher.local_map_tables(scene, dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        mean_shared = None
        for nq in batches:
            frame0, count, last = up(scene["frameMp"][:nq]), up(scene["count"][:nq]), up(scene["lastKf"][:nq])
            frame = frame0.clone()
            out = m.update_local_map(tables, frame, count, last, True, kf_out=128, mp_cap=8192)
            gat = m.gather_local_map_points(tables, out["localMp"], out["nLocalMp"])

            def call():
                frame.copy_(frame0)
                m.update_local_map(tables, frame, count, last, True, out=out)

            call()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            upd, gth = [], []
            for _ in range(reps):
                frame.copy_(frame0)
                torch.cuda.synchronize()
                ev[0].record()
                m.update_local_map(tables, frame, count, last, True, out=out)
                ev[1].record()
                m.gather_local_map_points(tables, out["localMp"], out["nLocalMp"], out=gat)
                ev[2].record()
                torch.cuda.synchronize()
                upd.append(ev[0].elapsed_time(ev[1]))
                gth.append(ev[1].elapsed_time(ev[2]))
            nk, nm, ov = out["nLocalKf"].cpu().numpy(), out["nLocalMp"].cpu().numpy(), out["overflow"].cpu().numpy()
            t0, oms, done, same = time.perf_counter(), 0.0, 0, True
            tab = oracle._tables(scene)
            for q in range(nq):
                if time.perf_counter() - t0 > oracle_limit_s:
                    break
                w = oracle.update(scene, q, True, tab)
                oms += oracle.last_ms()
                done += 1
                same = same and len(w["localKf"]) == nk[q] and len(w["localMp"]) == nm[q]
            if mean_shared is None:
                cv = scene["covis"][:64]
                rows = [set(r[r >= 0].tolist()) for r in scene["kfMp"]]
                mean_shared = float(np.mean([len(rows[k] & rows[n]) for k in range(len(cv)) for n in cv[k] if n >= 0]))
            res[f"kf{nkf}_q{nq}"] = dict(nmp=int(scene["nmp"]), local_kf_mean=float(nk.mean()), local_mp_mean=float(nm.mean()), overflow=int(ov.any()),
                                         shared_per_covisible_pair=mean_shared, update_ms_median=float(np.median(upd)), update_ms_min=float(np.min(upd)),
                                         gather_ms_median=float(np.median(gth)), oracle_frames=done, oracle_ms_per_frame=oms / max(done, 1),
                                         oracle_ms_batch=oms / max(done, 1) * nq, lengths_equal_oracle=bool(same))
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    main(reps=a.reps)
