"""The corpus of the whole-map bundle adjustment's tests (tests/test_global_ba_cpu.py selects it on the CPU, tests/test_global_ba_gpu.py runs it):
every camera x kernel setting x count of free keyframes, the two shapes of the envelope with and without loop points, a scene on, one below
and one above every tier constant of the kernels, and the named scenes, each with the CPU oracle's result computed once per build."""
import functools

import numpy as np

import global_ba_oracle as go
from morb_slam_amd.synth import make_global_ba_problem

CAMS = ("mix", "mono", "kb8")          # pinhole monocular + stereo, pinhole monocular only, KannalaBrandt8 rig with right-camera edges
_CAM_KW = {"mix": dict(mono_frac=0.3), "mono": dict(mono_frac=1.0), "kb8": dict(kb8=True)}
# the tier constants of csrc/global_ba.hip
ROWS_PER_PASS = 42                     # GBA_ROWS: covering rows (the diagonal block's among them) one pass of csrc/envelope_ldlt.h's envelope_factor takes
LDS_PANEL = 64                         # GBA_STAGE: blocks of a column's own row envelope_factor stages in LDS at a time
CHUNK = 64                             # GBA_CHUNK: Schur contributions to one envelope block added by one lane

# KannalaBrandt8::project takes theta and psi from atan2f, so chi2 is a staircase of ~1e-5 px steps in the estimate: a change of the rounding
# convention that moves an estimate by 1e-12 can put one edge on the next step, after which the LM paths part by ~1e-7.  Seeds on which a
# third build of the oracle (x87 arithmetic, tests/test_global_ba_cpu.py) takes such a step were replaced here, on the CPU, by the first
# of seed + 1000 k on which the three builds agree to 1e-10 in chi2.
_RESEED = {251: 1251, 310: 1310, 311: 2311, 312: 1312, 313: 3313}
# a case = (camera, keyframes, reach, points, loop points, robust, iterations, seed, extra keywords as a sorted tuple of pairs); one keyframe is
# fixed unless the extras say otherwise
# 1, 2, 3 free keyframes
SMALL = tuple((cam, nf + 1, 3, 40, 0, rob, 10, _RESEED.get(200 + 3 * i, 200 + 3 * i), ()) for i, (cam, rob, nf) in
              enumerate((c, r, f) for c in CAMS for r in (0, 1) for f in (1, 2, 3)))
# reach 1: Schur off-diagonal blocks between neighbours only; reach 30: every row covers every column; loop points give the long rows
SHAPES = tuple((cam, 30, reach, 300, loops, (i + k) & 1, 10, _RESEED.get(300 + 5 * i + k, 300 + 5 * i + k), ()) for i, cam in enumerate(CAMS)
               for k, (reach, loops) in enumerate(((1, 0), (1, 6), (30, 0), (6, 6))))
_FULL = (("obs_frac", 1.0),)           # every keyframe sees every point: a full envelope, every block with one contribution per point
# 40 | 41 | 42 rows below column 0: 41, 42 and 43 covering rows with the diagonal block's — one below, on and one above ROWS_PER_PASS
ROWS_EDGE = tuple(("mix", nf + 1, nf + 1, 60, 0, 0, 10, 41, _FULL) for nf in (ROWS_PER_PASS - 1, ROWS_PER_PASS, ROWS_PER_PASS + 1))
# the last row's own envelope holds 63 | 64 | 65 blocks in front of its diagonal block: one below, on and one above LDS_PANEL
PANEL_EDGE = tuple(("mix", nf + 1, nf + 1, 60, 0, 0, 10, 42, _FULL) for nf in (LDS_PANEL, LDS_PANEL + 1, LDS_PANEL + 2))
# two free keyframes that both see all of 63 | 64 | 65 points: every envelope block has that many contributions
CHUNK_EDGE = tuple((cam, 3, 3, n, 0, rob, 10, 43, _FULL) for cam, rob in (("mix", 0), ("kb8", 1)) for n in (CHUNK - 1, CHUNK, CHUNK + 1))
LARGE = (("mix", 120, 8, 2000, 10, 0, 10, 6, ()),)       # the size limit of the corpus: ~14 k edges
# the named scenes ("the named scenes do what their names say" in tests/test_global_ba_cpu.py); seeds found on the CPU
SPARSE_POINTS = ("mix", 14, 4, 100, 3, 0, 10, 7, (("fixed_only_points", 3), ("mono_single_points", 3), ("single_free_points", 3)))
SPARSE_POINTS_KB8 = ("kb8", 14, 4, 100, 3, 1, 10, 7, (("fixed_only_points", 3), ("mono_single_points", 3), ("single_free_points", 3)))
IDLE = ("mix", 14, 4, 100, 0, 0, 10, 9, (("idle_kf", 5), ("idle_points", 2)))
TWO_FIXED = ("mix", 14, 4, 100, 2, 1, 10, 10, (("n_fixed", 2),))
ONE_ITERATION = ("mix", 14, 4, 100, 0, 0, 1, 8, ())
# a noise-free KannalaBrandt8 scene that starts at the truth: the projection's atan2f makes chi2 a staircase, so the optimisation ends on
# rejected trials (ten in a row, or a step too small to move chi2: rho == 0)
AT_TRUTH = ("kb8", 12, 4, 120, 0, 0, 10, 3, (("at_truth", True),))
# a point 2e-38 in front of a free keyframe's focal plane with an information of 3e38: its Hessian block overflows in the inversion, every
# factorisation meets a NaN pivot, ten trials are rejected and nothing moves
FACTOR_FAILS = ("mix", 12, 4, 120, 0, 0, 10, 4, (("near_plane_point", True),))
FACTOR_FAILS_ROBUST = ("mix", 12, 4, 120, 0, 1, 10, 4, (("near_plane_point", True),))
NAMED = (SPARSE_POINTS, SPARSE_POINTS_KB8, IDLE, TWO_FIXED, ONE_ITERATION, AT_TRUTH, FACTOR_FAILS, FACTOR_FAILS_ROBUST)
CASES = SMALL + SHAPES + ROWS_EDGE + PANEL_EDGE + CHUNK_EDGE + LARGE + NAMED
# cases on which the two builds of the oracle part ways (stats, or outputs beyond 1e-6): they turn on the rounding of a sum and test no kernel
LEFT_OUT = frozenset()

# The largest relative difference of chi2 (before or after) between the oracle's two builds over the corpus, as tests/test_global_ba_cpu.py's
# test_corpus_selection measures and pins it (profiles/r19/README.md); the bound on the device's chi2 is ten times that, as the two pose
# graphs took it, above a floor of 1e-6: observations are floats of some hundred pixels (half an ulp: 1.5e-5 px), so the chi2 of a few
# hundred edges at the truth is rounding noise of that size.
CHI2_SPREAD = 1.1e-9                    # measured: 1.071e-9
CHI2_MARGIN = 10 * CHI2_SPREAD
CHI2_FLOOR = 1e-6


@functools.lru_cache(maxsize=None)
def scene(case):
    cam, n_kf, reach, n, loops, _rob, _its, seed, extra = case
    kw = dict(_CAM_KW[cam])
    kw.update(dict(extra))
    return make_global_ba_problem(n_kf, reach, n, loops, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def case_oracle(case, flags=go.DEFAULT_FLAGS):
    return go.run(scene(case), n_iterations=case[6], robust=bool(case[5]), flags=flags)


def case_id(case):
    return "-".join(str(x) for x in case[:8]) + ("-" + "-".join(k for k, _ in case[8]) if case[8] else "")


def structure(p):
    """The reduced system of a problem, worked out here from the edge list alone: col [nKF] (block row, -1: fixed or without an edge),
    rowFirst [n], and the number of Schur contributions of every envelope block {(row, column): count}."""
    nKF = len(p["kfPose"])
    used = np.zeros(nKF, bool); used[p["eKF"]] = True
    col = np.full(nKF, -1)
    free = np.flatnonzero(used & (p["kfFixed"] == 0))
    col[free] = np.arange(len(free))
    first = list(range(len(free)))
    count = {}
    for m in np.unique(p["eMP"]):
        rows = sorted(set(int(col[k]) for k in p["eKF"][p["eMP"] == m] if col[k] >= 0))
        for i, a in enumerate(rows):
            first[a] = min(first[a], rows[0])
            for b in rows[:i + 1]:
                count[(a, b)] = count.get((a, b), 0) + 1
    return col, np.array(first), count
