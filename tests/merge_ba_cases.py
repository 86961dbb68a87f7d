"""The corpus of the welding bundle adjustment's tests (tests/test_merge_ba_cpu.py selects it on the CPU, tests/test_merge_ba_gpu.py runs it):
every camera x window shape x point count of the issue's grid, the chunk-edge scene and the named scenes, each with the CPU oracle's result
computed once per build."""
import functools

import merge_ba_oracle as mo
from morb_slam_amd.synth import make_merge_ba_problem

CAMS = ("mix", "mono", "kb8")          # pinhole monocular + stereo, pinhole monocular only, KannalaBrandt8 left camera
FREE = (1, 3, 27, 28)                  # 27 | 28: the LDS-resident and the global-memory LDL^T (dense_ldlt.h)
FIXED = (1, 4)
POINTS = (60, 300)
_CAM_KW = {"mix": dict(mono_frac=0.3), "mono": dict(mono_frac=1.0), "kb8": dict(kb8=True)}

# a case = (camera, free keyframes, fixed keyframes, points, seed, extra keywords as a sorted tuple of pairs)
GRID = tuple((cam, nf, nx, n, 100 + 7 * i, ()) for i, (cam, nf, nx, n) in
             enumerate((c, f, x, n) for c in CAMS for f in FREE for x in FIXED for n in POINTS))
# keyframes 0, 1, 2 with exactly 63, 64 and 65 edges: one short of, exactly, and one beyond a 64-edge chunk
CHUNK_EDGE = tuple((cam, 4, 3, 300, 11, (("kf_edges", ((0, 63), (1, 64), (2, 65))),)) for cam in CAMS)
# the named scenes ("scene power" in tests/test_merge_ba_cpu.py); seeds found on the CPU.  REJECTED_LAST is a noise-free KannalaBrandt8 scene that
# starts at the truth: the projection's atan2f makes chi2 a staircase of ~1e-5 px, so round 1 converges at once and ends on rejected trials
# (ten in a row, or a step too small to move chi2: rho == 0).  The other three draw a point with gross observations only, a free keyframe with
# gross observations only, and a free keyframe whose own pose error five robust iterations do not remove.
REJECTED_LAST = ("kb8", 1, 4, 60, 37, (("kf_deg", 0.0), ("kf_trans", 0.0), ("noise_px", 0.0), ("outlier_frac", 0.0), ("point_noise", 0.0),
                                     ("rigid_deg", 0.0), ("rigid_trans", 0.0)))
POINT_DROPS = ("mix", 3, 4, 300, 21, (("bad_points", 3),))
KEYFRAME_DROPS = ("mix", 4, 4, 300, 22, (("bad_kf", 1),))
STALE_CHI2 = ("mix", 5, 4, 300, 23, (("stuck_kf", 2),))
NAMED = (REJECTED_LAST, POINT_DROPS, KEYFRAME_DROPS, STALE_CHI2)
CASES = GRID + CHUNK_EDGE + NAMED
# cases on which the two builds of the oracle part ways (stats, flags, or outputs beyond 1e-6): they turn on the rounding of a sum and test no kernel
LEFT_OUT = frozenset()


@functools.lru_cache(maxsize=None)
def scene(case):
    cam, nf, nx, n, seed, extra = case
    kw = dict(_CAM_KW[cam])
    for k, v in extra:
        kw[k] = dict(v) if k == "kf_edges" else v
    return make_merge_ba_problem(nf, nx, n, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def case_oracle(case, flags=mo.DEFAULT_FLAGS):
    return mo.run(scene(case), flags=flags)


def case_id(case):
    return "-".join(str(x) for x in case[:5]) + ("-" + "-".join(k for k, _ in case[5]) if case[5] else "")
