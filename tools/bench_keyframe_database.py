#!/usr/bin/env python3
"""Timing of the KeyFrameDatabase queries on MI355X (morb_detect_n_best_candidates_batch, morb_detect_relocalization_candidates_batch):
pools of 2000 and 10000 keyframes of about 1200 words over a vocabulary of 10^6 words, 1 and 64 queries per call: device time between
events per call after warm-up, the pool resident, beside the CPU oracle (tests/native/keyframe_database_oracle.cc, one thread, its
inverted file built beforehand) on the same queries.  Prints one JSON line; numbers only, no threshold."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import keyframe_database_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.synth import keyframe_database_connected_csr, make_keyframe_database_scene


def main(reps=20, sizes=(2000, 10000), batches=(1, 64)):
    m = ORBmatcher(0.8, True)
    oracle.lib()   # compiled before any timing
    dev = "cuda:0"
    res = {}
    for nimg in sizes:
        scene = make_keyframe_database_scene(seed=7, nKF=nimg, nwords_voc=1000000, words_per_kf=(1100, 1300), nmaps=2, cap=1300, ncovis=10,
                                             nplaces=max(nimg // 40, 1), place_words=3000, erased_frac=0.02, bad_frac=0.02)
        pick = np.random.default_rng(1).choice(nimg, max(batches), replace=False).astype(np.int32)
        scene["db_rank"][pick] = -1   # the queries are keyframes that have not been added yet, as in LoopClosing
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        bow = (up(scene["word"]), up(scene["value"]), up(scene["count"]))
        rank, covis, mapId, flags = up(scene["db_rank"]), up(scene["covis"]), up(scene["map_id"]), up(scene["flags"])
        db = oracle.Database(scene)
        for nq in batches:
            queries = pick[:nq]
            cs, cn = keyframe_database_connected_csr(scene, queries)
            d_q, d_cs, d_cn, d_qm = up(queries), up(cs), up(cn), up(scene["map_id"][queries])
            calls = {"n_best": lambda: m.DetectNBestCandidates(d_q, bow, rank, d_cs, d_cn, covis, mapId, flags, 3),
                     "reloc": lambda: m.DetectRelocalizationCandidates(d_q, d_qm, bow, rank, covis, mapId)}
            for name, call in calls.items():
                out = call()
                call()
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                launch = []
                for _ in range(reps):
                    ev0.record()
                    call()
                    ev1.record()
                    torch.cuda.synchronize()
                    launch.append(ev0.elapsed_time(ev1))
                words = out[4 if name == "n_best" else 2].cpu().numpy()
                zeros = np.zeros(nimg, np.float32)
                t0 = time.perf_counter()
                ncand = 0
                for q in queries:
                    db.set_scores(int(name == "reloc"), zeros)
                    if name == "n_best":
                        lo, me, _ = db.detect_n_best(q, 3)
                        ncand += len(lo) + len(me)
                    else:
                        ncand += len(db.detect_reloc(q, scene["map_id"][q])[0])
                oracle_ms = (time.perf_counter() - t0) * 1e3
                got = int(out[1].sum() + out[3].sum()) if name == "n_best" else int(out[1].sum())
                res[f"{name}_kf{nimg}_q{nq}"] = dict(stamped_mean=float((words > 0).sum(1).mean()), candidates=got, oracle_candidates=ncand,
                                                    call_ms_median=float(np.median(launch)), call_ms_min=float(np.min(launch)),
                                                    oracle_ms=oracle_ms)
        del db
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
