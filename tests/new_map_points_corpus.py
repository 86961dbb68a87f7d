"""The seeded corpus of the CreateNewMapPoints tests: four scenes of morb_slam_amd.synth.make_new_map_points_scene, one per kind (mono,
stereo features in keyframe 1, in keyframe 2, KannalaBrandt8 rig), four keyframe pairs each (16 pairs), cap 96 and 40 to 96 synthetic
keypoints per image: no extraction is needed.  The oracle's results are computed once per process and shared."""
import functools

import numpy as np

import new_map_points_oracle as oracle
from morb_slam_amd.synth import NEW_MAP_POINT_KINDS, make_new_map_points_scene

CAP, PAIRS = 96, 4


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(make_new_map_points_scene(seed=3, kind=k, npairs=PAIRS, cap=CAP, nfeat=(40, 96)) for k in NEW_MAP_POINT_KINDS)


@functools.lru_cache(maxsize=None)
def results(flags=oracle.DEFAULT_FLAGS):
    """Per scene: the oracle's dict(status, stats, tables, hasMP); read-only."""
    out = []
    for s in scenes():
        r = oracle.run(oracle.arrays_of_scene(s), flags=flags)
        for a in [r["status"], r["stats"], r["hasMP"], *r["tables"].values()]:
            a.setflags(write=False)
        out.append(r)
    return tuple(out)


def status_histogram():
    h = np.zeros(32, np.int64)
    for s, r in zip(scenes(), results()):
        matched = s["match12"] >= 0
        h += np.bincount(r["status"][matched], minlength=32)
    return h
