#!/usr/bin/env python3
"""Timing of CreateNewMapPoints on MI355X (morb_create_new_map_points_batch): milliseconds per call, inputs resident, for 1 pair, the 10
neighbour ranks of one keyframe (10 calls of one pair), 256 pairs at cap 1200 and 256 pairs at cap 4500, each beside the one-thread
CPU oracle (tests/native/new_map_points_oracle.cc) on the same pairs; and tracking.LocalMappingChain.step (search, create, Fuse per
rank) beside the same searches and Fuse without the create stage.  A call uploads its poses and waits for that copy, so the wall time
of a call is reported beside the device time between events.  Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import new_map_points_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.capi import KP_DTYPE
from morb_slam_amd.synth import (make_local_mapping_scene, make_new_map_points_scene, new_map_points_frame_params,
                                 pack_new_map_points_scene)
from morb_slam_amd.tracking import LocalMappingChain

DEV = "cuda:0"


def tiled(scene, times):
    """The scene's pairs `times` times over, every copy with images of its own."""
    s = dict(scene, npairs=scene["npairs"] * times, nimg=scene["nimg"] * times)
    for k in ("count", "nLeft", "xy", "xyRaw", "octave", "desc", "uRight", "depth", "node", "match12", "poses", "kf2First", "X", "category", "R12",
              "t12", "ep"):
        s[k] = np.concatenate([scene[k]] * times)
    s["img1"], s["img2"] = np.arange(0, s["nimg"], 2, dtype=np.int32), np.arange(1, s["nimg"], 2, dtype=np.int32)
    return s


def timed(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev0.elapsed_time(ev1))
    return dict(device_ms_median=float(np.median(dev)), wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)))


def create_case(m, scene, calls, reps):
    """calls: lists of pair indices, one launch each."""
    t = pack_new_map_points_scene(scene, DEV)
    P = new_map_points_frame_params(scene)
    tables = m.new_map_point_tables(scene["npairs"], scene["cap"], DEV)
    sub = [(torch.from_numpy(np.asarray(c, np.int64)).to(DEV), np.asarray(c)) for c in calls]
    args = [(t["img1"][i], t["img2"][i], t["match12"][i].contiguous(), scene["poses"][h], scene["kf2First"][h], t["row"][i]) for i, h in sub]
    outs = [(torch.empty((len(h), scene["cap"]), dtype=torch.int32, device=DEV), torch.empty((len(h), 5), dtype=torch.int32, device=DEV)) for _, h in sub]

    def run():
        t["hasMP"].zero_()
        for (i1, i2, m12, poses, first, row), o in zip(args, outs):
            m.CreateNewMapPoints(P, i1, i2, t["kps"], t["desc"], t["count"], m12, poses, first, row, tables, t["hasMP"],
                                 ratioFactor=scene["ratioFactor"], mbFarPoints=True, mThFarPoints=scene["thFarPoints"], out=o)
    run()
    torch.cuda.synchronize()
    created = int(sum(int(o[1][:, 0].sum()) for o in outs))
    r = timed(run, reps)
    A = oracle.arrays_of_scene(scene)
    t0 = time.perf_counter()
    o = oracle.run(A)
    r.update(oracle_ms=(time.perf_counter() - t0) * 1e3, pairs=scene["npairs"], launches=len(calls), cap=scene["cap"],
             matches=int((scene["match12"] >= 0).sum()), created=created, oracle_created=int(o["stats"][:, 0].sum()))
    return r


def chain_case(reps, B=32, K=4, cap=1200, npts=1000):
    sc = make_local_mapping_scene(seed=1, B=B, K=K, cap=cap, npts=npts)
    P = new_map_points_frame_params(sc)
    kps = np.zeros((sc["nimg"], cap), KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["octave"] = sc["xy"][..., 0], sc["xy"][..., 1], 31.0, sc["octave"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ch = LocalMappingChain(P, t(kps.view(np.uint8).reshape(sc["nimg"], cap, 28)), t(sc["desc"]), t(sc["node"]), t(sc["count"]), sc)

    def full():
        ch.hasMP.zero_()
        ch.step()

    def searches_only():   # what KeyframeSearches.step runs per rank: SearchForTriangulation and Fuse, the table left as it is
        ch.hasMP.zero_()
        st = ch.stream.cuda_stream
        with torch.cuda.stream(ch.stream):
            for k in range(ch.K):
                h = ch.host[k]
                ch.m.SearchForTriangulation(ch.P, ch.img1, ch.img2[k], ch.kps, ch.desc, ch.node, ch.count, ch.hasMP, None, h["R12"], h["t12"],
                                            h["ep"], False, False, out=ch.tri[k], stream=st)
            for k in range(ch.K):
                ch.m.Fuse(ch.P, ch.img2[k], ch.kps, ch.desc, ch.count, None, ch.Tcw7[k], ch.Ow[k], ch.nMP, ch.valid[k], ch.tables["Xw"],
                          ch.tables["normal"], ch.tables["maxDist"], ch.tables["minDist"], ch.tables["desc"], ch.th, out=ch.fused[k], stream=st)
    full()
    torch.cuda.synchronize()
    created = int(sum(int(c[1][:, 0].sum()) for c in ch.created))
    r = dict(keyframes=B, ranks=K, cap=cap, created=created, chain=timed(full, reps), search_and_fuse=timed(searches_only, reps))
    ch.close()
    return r


def main(reps=10):
    m = ORBmatcher(0.6, False, device=0)
    oracle.lib()   # compiled before any timing
    res = {}
    s1200 = make_new_map_points_scene(seed=1, kind="mono", npairs=16, cap=1200, nfeat=(1000, 1200))
    s4500 = make_new_map_points_scene(seed=2, kind="mono", npairs=8, cap=4500, nfeat=(3800, 4500))
    res["pair_1"] = create_case(m, tiled(s1200, 1), [[0]], reps)
    res["ranks_10"] = create_case(m, tiled(s1200, 1), [[k] for k in range(10)], reps)
    res["pairs_256_cap1200"] = create_case(m, tiled(s1200, 16), [list(range(256))], reps)
    res["pairs_256_cap4500"] = create_case(m, tiled(s4500, 32), [list(range(256))], reps)
    # (the oracle of the first two cases ran the scene's 16 pairs: scale it to the pairs the device ran)
    res["pair_1"]["oracle_ms"] *= 1 / 16
    res["ranks_10"]["oracle_ms"] *= 10 / 16
    res["local_mapping_chain"] = chain_case(reps)
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
