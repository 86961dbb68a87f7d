"""The corpus of MergeInertialBA problems shared by tests/test_merge_inertial_ba_cpu.py (which selects it on the oracle alone) and
tests/test_merge_inertial_ba_gpu.py (which runs the kept cases against the oracle).  A case = (name, keyword arguments of
morb_slam_amd.synth.make_merge_inertial_ba_problem).  (15-dof, 6-dof) free keyframes = (1 + n_cur + n_merge, n_cov)."""
import functools

import numpy as np

CAMERAS = {"mix": dict(mono_frac=0.3), "mono": dict(mono_frac=1.0), "kb8": dict(kb8=True)}
# (15-dof, 6-dof) -> (n_cur, n_merge, n_cov): P = 30 smallest | 51 both widths | 162 last on the LDS-resident LDL^T | 165 twice: first on the
# global-memory solver | 375 the reference's largest graph
SIZES = {(2, 0): (0, 1, 0), (3, 1): (1, 1, 1), (10, 2): (5, 4, 2), (9, 5): (4, 4, 5), (11, 0): (5, 5, 0), (13, 30): (6, 6, 30)}


def _size(n15n6, **kw):
    n_cur, n_merge, n_cov = SIZES[n15n6]
    return dict(n_cur=n_cur, n_merge=n_merge, n_cov=n_cov, **kw)


def _cases():
    out = []
    for cam, ckw in CAMERAS.items():
        for n15n6 in SIZES:
            big = n15n6 == (13, 30)
            for seed, npts in ((0, 300),) if big else ((0, 60), (1, 300)):
                out.append((f"{cam}-{n15n6[0]}x{n15n6[1]}-s{seed}", _size(n15n6, n_points=npts, seed=seed, **ckw)))
    return out


# named scenes: what each is for is asserted in test_merge_inertial_ba_cpu.py::test_scene_power
NAMED = [
    # one 15-dof keyframe (1) and one 6-dof keyframe (4) with exactly 63 / 64 / 65 edges: the edges of k_iba_kf's 64-edge chunks
    ("chunk63", _size((3, 1), n_points=300, seed=3, kf_edges={1: 63, 4: 63})),
    ("chunk64", _size((3, 1), n_points=300, seed=4, kf_edges={1: 64, 4: 64})),
    ("chunk65", _size((3, 1), n_points=300, seed=5, kf_edges={1: 65, 4: 65})),
    ("kicked-link", _size((3, 1), n_points=60, seed=6, vel_kick={1: 1.0})),                      # a link far above the Huber bar
    ("shifted-fixed", dict(n_cur=2, n_merge=2, n_cov=2, n_points=60, seed=1, fixed_shift=5.0)),     # rejected trials on the way
    ("behind", _size((3, 1), n_points=60, seed=7, n_behind=4, mono_frac=1.0)),                     # negative depths with a small chi2
    ("behind-kb8", _size((3, 1), n_points=60, seed=7, n_behind=4, kb8=True)),
    ("cov-only-points", _size((10, 2), n_points=60, seed=8, n_cov_only=5)),                        # points seen by pose-only keyframes alone
    ("single-head", _size((2, 0), n_points=60, seed=9)),                                           # chain A = a free head with no link
    ("observers", _size((3, 1), n_points=60, seed=10, n_fixed_vis=3)),                             # kind 2 beside kinds 0, 1, 3
    # chain B begins with two FIXED keyframes joined by a link: a constant K of the robust chi2.  10 km apart, K ~ 3e9 is a thousand times what
    # the rest of the graph can gain, so three iterations in a row gain less than 0.1 % and the stagnation rule ends the solve; 1e20 m apart,
    # K ~ 3e25 has an ulp of 4e9, every sum IS K, the first trial's rho is exactly 0 and the solve ends on that rejected trial
    ("stagnates", _size((3, 1), n_points=60, seed=11, fixed_pair=1e4)),
    ("stagnates-kb8", _size((3, 1), n_points=60, seed=11, fixed_pair=1e4, kb8=True)),
    ("ends-rejected", _size((3, 1), n_points=60, seed=12, fixed_pair=1e20)),
]
CASES = _cases() + NAMED
NAMED_NAMES = tuple(n for n, _ in NAMED)
# cases on which the oracle's two builds (flags, summation order) disagree in stats3, erase flags or beyond 1e-6: not compared on the GPU.
# Selected on the oracle alone by test_merge_inertial_ba_cpu.py::test_corpus_selection, which also holds this list to what it finds.
LEFT_OUT = ()
KEPT = tuple(n for n, _ in CASES if n not in LEFT_OUT)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(problem, preintegrations [nI, 310]) of a case; the preintegrations come from the CPU oracle of IMU::Preintegrated."""
    from morb_slam_amd.synth import make_merge_inertial_ba_problem
    p = make_merge_inertial_ba_problem(**dict(CASES)[name])
    return p, preintegrate(p)


def preintegrate(p):
    import oracle_lib as orc
    from morb_slam_amd.synth import imu_calib_diagonals
    nga, walk = imu_calib_diagonals()
    return np.stack([orc.imu_preintegrate(p["bias"], nga, walk, p["acc"][a:b], p["gyro"][a:b], p["dt"][a:b])
                     for a, b in zip(p["imuStart"][:-1], p["imuStart"][1:])])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The default build's result on a case (computed once, shared by the tests; treat it as read-only)."""
    import merge_inertial_ba_oracle as mo
    p, pre = problem(name)
    return mo.run(p, pre)
