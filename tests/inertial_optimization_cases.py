"""The scenes the InertialOptimization tests share: tests/test_inertial_optimization_gpu.py compares the kernel with the CPU oracle on them,
tests/test_inertial_optimization_cpu.py checks that the oracle's Levenberg-Marquardt path on each of them does not hang on the last bits
of a sum (two builds of the oracle, the links summed in both orders).  A case whose path does is listed in LEFT_OUT and skipped by both."""
import numpy as np

import inertial_optimization_oracle as io
import oracle_lib as orc
from morb_slam_amd.synth import IMU_FREQ, imu_calib_diagonals, make_inertial_optimization_problem

LDS_EDGE = 192   # csrc/inertial_optimization.hip: IO_LDS_KF — a problem of up to 192 keyframes keeps its chain in LDS

# mode 0: (mono, priorG, priorA, bFixedVel)
VARIANTS = {"mono": (True, 1e2, 1e10, False), "stereo": (False, 1e2, 1e5, False), "mono_noprior": (True, 0.0, 0.0, False),
            "stereo_noprior": (False, 0.0, 0.0, False), "mono_fixedvel": (True, 1e2, 1e10, True)}
SMALL, LARGE = (3, 10, 11), (64, 65, LDS_EDGE, LDS_EDGE + 1)
MODE0_CASES = [(n, v, s) for n in SMALL for v in VARIANTS for s in range(3)] + [(n, v, 0) for n in LARGE for v in VARIANTS]
# (n, variant, seed) whose (iterations, trials) differ between the two oracle builds: the LM path turns on the rounding of a sum there
LEFT_OUT = set()


def preintegrate(p, freq=IMU_FREQ):
    """The oracle's preintegrations of a scene's links: [n, 310] f32 (row 0: keyframe 0's unused record)."""
    nga, walk = imu_calib_diagonals(freq)
    s = p["imuStart"]
    return np.stack([orc.imu_preintegrate(p["bias"], nga, walk, p["acc"][a:b], p["gyro"][a:b], p["dt"][a:b]) for a, b in zip(s[:-1], s[1:])])


_cache = {}


def scene(key, **kw):
    """make_inertial_optimization_problem(**kw) with its preintegrations, made once per key."""
    if key not in _cache:
        p = make_inertial_optimization_problem(**kw)
        _cache[key] = (p, preintegrate(p))
    return _cache[key]


def mode0_scene(n, variant, seed):
    mono, pg, pa, fixed = VARIANTS[variant]
    return scene(("m0", n, variant, seed), n_kf=n, seed=seed, mono=mono, s_true=1.2 if mono else 1.0, prior_g=pg, prior_a=pa, fixed_vel=fixed,
                 n_imu=20)


def mode1_scene(n, seed=0, **kw):
    """A map that is already initialised: the world is gravity-aligned and metric; the gyro bias moved a little since."""
    p, pre = scene(("m1", n, seed, tuple(sorted(kw.items()))), n_kf=n, seed=seed, mono=False, s_true=1.0, rwg_deg=0.0, n_imu=20, **kw)
    return p, pre


def mode2_scene(n, seed=0, outliers=()):
    """ScaleRefinement: Rwg and the scale start off the optimum of a mono map; velocities and biases are fixed."""
    p, pre = scene(("m2", n, seed, tuple(outliers)), n_kf=n, seed=seed, mono=True, s_true=1.1, n_imu=20, outlier_links=tuple(outliers))
    p = dict(p)
    g = p["global16"].copy()
    g[9] = 1.0
    g[10:13] = p["bg_true"]; g[13:16] = p["ba_true"]
    p["global16"] = g
    p["kfState"] = p["kfState"].copy()
    p["kfState"][:, 12:15] = p["v_true"]
    return p, pre


_oracle = {}


def oracle(key, p, pre, mode, flags=io.DEFAULT_FLAGS, **kw):
    k = (key, mode, tuple(flags))
    if k not in _oracle:
        _oracle[k] = io.run(p, pre, mode, flags=flags, **kw)
    return _oracle[k]
