"""The corpus of the inertial whole-map bundle adjustment's tests (tests/test_full_inertial_ba_cpu.py selects it on the CPU,
tests/test_full_inertial_ba_gpu.py runs it).  A case = (name, keyword arguments of morb_slam_amd.synth.make_full_inertial_ba_problem, its).

The gauge.  FullInertialBA fixes nothing at its call sites: yaw and translation of the whole map are held by lambda = 1e-5 alone, the
rounding noise of the right-hand side along those four directions is divided by it, and from the second iteration on (lambda falls by three
with every kept step) any two FP64 evaluations of the same algorithm — the oracle's two builds are two — part by 1e-4 .. 1 in the states
and, through the steps' nonlinearity, in chi2 and in the LM path (profiles/r20/README.md has the figures).  That is the reference's
conditioning, not a kernel's.  So the nothing-fixed gauge is the norm of the corpus over ONE iteration, where the builds agree to 1e-6: every
camera, size, shape, tier edge and the largest scene.  The LM path over 7 and 100 iterations — rejected trials, the stagnation rule, failed
factorisations — runs on the named scenes that fix the first keyframe (kind 1), where the builds agree to the last bit.  Links carry 100 IMU
samples (half a second): with 20 the information of a link is a hundred times larger and so is the noise along the gauge."""
import functools

import numpy as np

CAMS = ("mix", "mono", "kb8")          # pinhole monocular + stereo, pinhole monocular only, KannalaBrandt8 rig with right-camera edges
_CAM_KW = {"mix": dict(mono_frac=0.3), "mono": dict(mono_frac=1.0), "kb8": dict(kb8=True)}
N_IMU = 100
# the tier constants of csrc/full_inertial_ba.hip
ROWS_PER_PASS = 85                     # FIBA_ROWS: covering rows (the diagonal block's among them) one pass of csrc/envelope_ldlt.h's envelope_factor takes
LDS_PANEL = 128                        # FIBA_STAGE: 3 x 3 blocks of a column's own row envelope_factor stages in LDS at a time
CHUNK = 64                             # FIBA_CHUNK: Schur contributions to one envelope block added by one lane

# seeds replaced on the CPU by the first of seed + 1000 k on which the oracle's two builds agree (tests/test_full_inertial_ba_cpu.py)
_RESEED = {119: 2119, 124: 1124, 126: 1126, 127: 3127, 129: 1129}


def _case(name, its, seed, cam="mix", **kw):
    d = dict(_CAM_KW[cam])
    d.update(kw)
    d.setdefault("n_imu", N_IMU)
    d["seed"] = _RESEED.get(seed, seed)
    return (name, tuple(sorted(d.items())), its)


# 1, 2 and 3 keyframes (no link, one link, two) x camera x bInit; nothing fixed — but beside the single keyframe, which has no link and is
# free in the pose only, stands one fixed observer (kind 2) that sees every point: one camera and the points it alone sees are all gauge,
# and the step is whatever the 3 x 3 inverses round to (on the device 6e-3 .. 1e-1 from the oracle, whose two builds agree)
SMALL = tuple(_case(f"small-{cam}-{n}kf-init{b}", 1, 100 + 10 * i + 3 * n + b, cam, n_kf=n, reach=3, n_points=40, init=bool(b),
                    observers=1 if n == 1 else 0, observer_frac=1.0)
              for i, cam in enumerate(CAMS) for n in (1, 2, 3) for b in (0, 1))
# reach 1: neighbours only; reach 30: every row covers every column; loop points give the long rows; bInit's shared row spans everything anyway
SHAPES = tuple(_case(f"shape-{cam}-reach{reach}-loop{loops}-init{b}", 1, 300 + 10 * i + 2 * k + b, cam, n_kf=30, reach=reach, n_points=300,
                     n_loop_points=loops, init=bool(b))
               for i, cam in enumerate(CAMS) for k, (reach, loops) in enumerate(((1, 0), (30, 0), (6, 6))) for b in (0, 1))
# a keyframe without IMU in the middle: kind 3, the chain cut there
CUT = (_case("cut-mix", 1, 400, "mix", n_kf=12, reach=4, n_points=120, no_imu=(5,)),
       _case("cut-kb8-init", 1, 401, "kb8", n_kf=12, reach=4, n_points=120, no_imu=(5,), init=True))
_FULL = dict(obs_frac=1.0)             # every keyframe sees every point: a full envelope
# 84 | 85 | 86 block rows cover column 0 (the diagonal block's among them): 16 keyframes of 5 rows + 2 of 2, 17 of 5, 16 of 5 + 3 of 2
ROWS_EDGE = (_case("rows-84", 1, 500, n_kf=18, reach=18, n_points=60, no_imu=(0, 17), **_FULL),
             _case("rows-85", 1, 501, n_kf=17, reach=17, n_points=60, **_FULL),
             _case("rows-86", 1, 502, n_kf=19, reach=19, n_points=60, no_imu=(0, 9, 18), **_FULL))
# the last row's envelope holds 127 | 128 | 129 blocks in front of its diagonal block: n = 128 (24 x 5 + 4 x 2), 129 (25 x 5 + 2 x 2), 130 (26 x 5)
PANEL_EDGE = (_case("panel-127", 1, 510, n_kf=28, reach=28, n_points=60, no_imu=(0, 9, 18, 27), **_FULL),
              _case("panel-128", 1, 511, n_kf=27, reach=27, n_points=60, no_imu=(0, 26), **_FULL),
              _case("panel-129", 1, 512, n_kf=26, reach=26, n_points=60, **_FULL))
# three keyframes that all see all of 63 | 64 | 65 points: every envelope block a point reaches has that many contributions
CHUNK_EDGE = tuple(_case(f"chunk-{n}-{cam}", 1, 520 + n + j, cam, n_kf=3, reach=3, n_points=n, init=bool(j), **_FULL)
                   for j, cam in enumerate(("mix", "kb8")) for n in (CHUNK - 1, CHUNK, CHUNK + 1))
LARGE = (_case("large-120", 1, 6, n_kf=120, reach=8, n_points=2000, n_loop_points=10),)      # the size limit of the corpus: ~14 k edges
# ---- the named scenes ("the named scenes do what their names say" in tests/test_full_inertial_ba_cpu.py) ----
# the first keyframe fixed with its IMU state (kind 1): the LM path over 7 (loop closing) and 100 (IMU initialisation) iterations
GAUGED = tuple(_case(f"gauged-{cam}-init{b}-its{its}", its, 600 + 10 * i + 2 * k + b, cam, n_kf=30, reach=6, n_points=300, n_loop_points=4,
                     n_fixed=1, init=bool(b))
               for i, cam in enumerate(CAMS) for k, its in enumerate((7, 100)) for b in (0, 1))
GAUGED_SMALL = tuple(_case(f"gauged-small-{n}kf-init{b}-its100", 100, 650 + 2 * n + b, n_kf=n, reach=3, n_points=40, n_fixed=1, init=bool(b))
                     for n in (2, 3) for b in (0, 1))
GAUGED_LARGE = _case("gauged-large-120-its7", 7, 6, n_kf=120, reach=8, n_points=2000, n_loop_points=10, n_fixed=1)
GAUGED_CUT = _case("gauged-cut-its7", 7, 660, n_kf=12, reach=4, n_points=120, no_imu=(5,), n_fixed=1)
FIXED_PAIR = _case("fixed-pair-its7", 7, 670, n_kf=14, reach=4, n_points=100, n_fixed=2)                  # a link between two kind-1 keyframes
FIXED_PAIR_INIT = _case("fixed-pair-init-its7", 7, 671, n_kf=14, reach=4, n_points=100, n_fixed=2, init=True)   # ... which still moves the shared biases
OBSERVERS = _case("observers-its7", 7, 672, n_kf=14, reach=4, n_points=100, n_fixed=1, observers=3)       # kind 2 beside kinds 0 and 1
IDLE = _case("idle-points", 1, 673, n_kf=14, reach=4, n_points=100, idle_points=2)
# a noise-free KannalaBrandt8 scene that starts at the truth: the projection's atan2f makes chi2 a staircase, trials get rejected
AT_TRUTH = _case("at-truth-kb8-its7", 7, 680, "kb8", n_kf=12, reach=4, n_points=120, n_fixed=1, at_truth=True)
AT_TRUTH_FREE = _case("at-truth-free-its1", 1, 681, "kb8", n_kf=12, reach=4, n_points=120, at_truth=True)
# a point 2e-38 in front of a keyframe's focal plane with an information of 3e38: its Hessian block does not survive the inversion, every
# factorisation meets a NaN pivot, ten trials are rejected and nothing moves
FACTOR_FAILS = _case("factor-fails-its7", 7, 690, n_kf=12, reach=12, n_points=120, n_fixed=1, near_plane_point=5, **_FULL)
FACTOR_FAILS_INIT = _case("factor-fails-init-its7", 7, 691, n_kf=12, reach=12, n_points=120, n_fixed=1, near_plane_point=5, init=True, **_FULL)
# ---- the call sites' own configuration: nothing fixed, 7 and 100 iterations.  The states drift along the gauge (above), so these are not
# compared state by state: the device's chi2 must fall, stand within ten times the builds' spread of the oracle's, and be the chi2 the oracle
# finds at the state the device returns (tests/test_full_inertial_ba_gpu.py::test_call_site_configuration)
FREE_PATH = tuple(_case(f"free-{cam}-init{b}-its{its}", its, 700 + b, cam, n_kf=30, reach=6, n_points=300, n_loop_points=4, init=bool(b))
                  for cam in CAMS for b in (0, 1) for its in (7, 100))
# the single keyframe as it stands alone: no link, free in the pose only, nothing fixed — one camera and its points are all gauge, the step is
# what the 3 x 3 inverses round to, and a third build of the oracle (x87 arithmetic) parts from the first by 1e-2 .. 4e-1 in the states and
# up to 3e-1 in chi2, as the device does (tests/test_full_inertial_ba_cpu.py::test_lone_keyframe_turns_on_rounding).  Held as FREE_PATH is.
LONE = tuple(_case(f"lone-{cam}-init{b}", 1, 100 + 10 * i + 3 + b, cam, n_kf=1, reach=3, n_points=40, init=bool(b))
             for i, cam in enumerate(CAMS) for b in (0, 1))
# largest difference of the final chi2, relative to max(1, chi2), between the oracle's two builds over FREE_PATH (measured 1.08e-3, free-mix-init1-its7, whose
# builds take 13 and 12 trials), and largest relative gap between the chi2 the oracle reports and the chi2 it finds at its own float outputs
# (measured 6.6e-7): the device is held to ten times each
FREE_CHI2_SPREAD = 1.1e-3
REEVAL_GAP = 7e-7
NAMED = GAUGED + GAUGED_SMALL + (GAUGED_LARGE, GAUGED_CUT, FIXED_PAIR, FIXED_PAIR_INIT, OBSERVERS, IDLE, AT_TRUTH, AT_TRUTH_FREE, FACTOR_FAILS,
                                 FACTOR_FAILS_INIT)
TIER = ROWS_EDGE + PANEL_EDGE + CHUNK_EDGE
CASES = SMALL + SHAPES + CUT + TIER + LARGE + NAMED
# cases on which the two builds of the oracle part ways (stats, or outputs beyond 1e-6): they turn on the rounding of a sum and test no
# kernel.  At most 3, none of them a tier-edge or a named scene (tests/test_full_inertial_ba_cpu.py::test_corpus_selection).
LEFT_OUT = frozenset()
KEPT = tuple(c for c in CASES if c[0] not in LEFT_OUT)

# The largest relative difference of chi2 (before or after) between the oracle's two builds over the kept cases, as
# tests/test_full_inertial_ba_cpu.py::test_corpus_selection measures and pins it (profiles/r20/README.md); the bound on the device's chi2 is
# ten times that, above a floor of 1e-6 as in the three earlier map-sized optimisers.
CHI2_SPREAD = 3.2e-6                    # measured: 3.113e-6
CHI2_MARGIN = 10 * CHI2_SPREAD
CHI2_FLOOR = 1e-6


def parting(a, b):
    """How far two results are apart: rotations, velocities and biases absolutely, positions and points relative to max(1, |.|) — a float's
    ulp at 14 m, the far end of the largest scene, is 9.5e-7.  (stats equal, distance)"""
    ka, kb = a["kfState"].astype(np.float64), b["kfState"].astype(np.float64)
    d = np.abs(ka - kb)
    d[:, 9:12] /= np.maximum(1.0, np.linalg.norm(ka[:, 9:12], axis=1))[:, None]
    pa, pb = a["mpPos"].astype(np.float64), b["mpPos"].astype(np.float64)
    dp = np.abs(pa - pb).max(1) / np.maximum(1.0, np.linalg.norm(pa, axis=1))
    db = np.abs(a["bias6"].astype(np.float64) - b["bias6"]).max()
    return a["stats4"].tolist() == b["stats4"].tolist(), float(max(d.max(), dp.max(), db))


def chi2_at(p, pre, result):
    """The robust chi2 the oracle finds at a result's state (its chi2 at entry of a call on that state)."""
    import full_inertial_ba_oracle as fo
    return float(fo.run(dict(p, kfState=result["kfState"], mpPos=result["mpPos"], bias6=result["bias6"]), pre, its=1)["chi2"][0])


def case_id(case):
    return case[0]


@functools.lru_cache(maxsize=None)
def scene(case):
    """(problem, preintegrations [nI, 310]) of a case; the preintegrations come from the CPU oracle of IMU::Preintegrated."""
    from morb_slam_amd.synth import make_full_inertial_ba_problem
    p = make_full_inertial_ba_problem(**dict(case[1]))
    return p, preintegrate(p)


def preintegrate(p):
    import oracle_lib as orc
    from morb_slam_amd.synth import imu_calib_diagonals
    nga, walk = imu_calib_diagonals()
    s = p["imuStart"]
    if not len(p["iKF1"]):
        return np.zeros((0, 310), np.float32)
    return np.stack([orc.imu_preintegrate(p["bias"], nga, walk, p["acc"][s[k]:s[k + 1]], p["gyro"][s[k]:s[k + 1]], p["dt"][s[k]:s[k + 1]])
                     for k in p["iKF1"]])


@functools.lru_cache(maxsize=None)
def case_oracle(case, flags=None):
    """The oracle's result on a case (computed once per build, shared by the tests; treat it as read-only)."""
    import full_inertial_ba_oracle as fo
    p, pre = scene(case)
    return fo.run(p, pre, its=case[2], flags=flags or fo.DEFAULT_FLAGS)


def structure(p):
    """The reduced system of a problem, worked out here from the edge and link lists alone: rows [nKF] (3 x 3 block rows of a keyframe in
    the system, 0: not in it), first [n] (the first block column of every block row, the shared biases' rows last), and the number of
    points every pair of keyframes of the system shares {(kf, kf'): count}, kf >= kf'."""
    kind, init = p["kfKind"], p["init"]
    seen = np.zeros(len(kind), bool); seen[p["eKF"]] = True
    rows = np.where(kind == 0, 3 if init else 5, np.where((kind == 3) & seen, 2, 0))
    start = np.concatenate([[0], np.cumsum(rows)])
    low = {k: k for k in np.flatnonzero(rows)}
    count = {}
    for m in np.unique(p["eMP"]):
        ks = sorted(set(int(k) for k in p["eKF"][p["eMP"] == m] if rows[k]))
        for i, a in enumerate(ks):
            low[a] = min(low[a], ks[0])
            for b in ks[:i + 1]:
                count[(a, b)] = count.get((a, b), 0) + 1
    linked = []
    for a, b in zip(p["iKF1"], p["iKF2"]):
        if rows[a] and rows[b]:
            low[max(a, b)] = min(low[max(a, b)], min(a, b))
        linked += [k for k in (a, b) if rows[k]]
    first = []
    for k in np.flatnonzero(rows):
        first += [int(start[low[k]])] * int(rows[k])
    if init and len(first):
        n = len(first)
        first += [int(start[min(linked)]) if linked else n] * 2
    return rows, np.array(first), count
