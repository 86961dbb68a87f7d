"""The corpus of the OptimizeEssentialGraph tests: small graphs of synth.make_essential_graph_problem, one or more per class of the solver's
and of Sim3::log's paths, each with the classes it stands for.  case_problem / case_oracle build and cache; the CPU test
(test_essential_graph_cpu.py::test_corpus_selection) runs every case through both builds of the oracle and checks that the two agree on
the Levenberg-Marquardt path of at least half the cases and of at least one case of every class: only those pin the GPU's path.
Every graph but n2 has a cycle whose measurements do not close, so its optimum has a residual: on a tree every error can be driven to zero,
and once chi2 is ~1e-30 each further decision compares rounding noise (N = 2 is a tree whatever one does: it starts at its optimum)."""
import functools

import numpy as np

import essential_graph_oracle as eo
from morb_slam_amd.synth import make_essential_graph_problem

PANEL = 32    # csrc/essential_graph.hip: EG_PANEL, blocks of a column's own row csrc/envelope_ldlt.h's envelope_factor stages in LDS at a time
LINES = 256   # ... EG_NT: lanes of the workgroup; a pass takes the block lines (7 per covering row) of 36 rows, 252

# name -> (classes, keyword arguments of the generator; "start" = "optimum": the oracle's result is the starting point)
CASES = {
    "n2": ({"n2", "long0", "band1"}, dict(n_kf=2, band=1, n_loop=0, loop_rot_deg=0, seed=1)),
    "n3": ({"n3", "long0"}, dict(n_kf=3, band=2, n_loop=0, seed=400, meas_noise=0.02)),   # a triangle whose measurements do not close
    "n9": ({"n9", "band3", "long_span"}, dict(n_kf=9, band=3, seed=5, n_points=12)),
    "n9_b": ({"n9", "band3"}, dict(n_kf=9, band=3, seed=15, n_points=5, loop_kf=2)),
    "panel_minus": ({"panel-1", "long_span"}, dict(n_kf=PANEL + 1, band=3, loop_kf=1, seed=6)),
    "panel": ({"panel", "long_span"}, dict(n_kf=PANEL + 2, band=3, loop_kf=1, seed=7)),
    "panel_plus": ({"panel+1", "long_span"}, dict(n_kf=PANEL + 3, band=3, loop_kf=1, seed=8, n_points=30)),
    "panel_plus_b": ({"panel+1", "panel", "panel-1", "long_span"}, dict(n_kf=2 * PANEL + 3, band=2, loop_kf=1, seed=28)),
    "two_passes": ({"lines>256", "long5"}, dict(n_kf=60, band=20, loop_kf=2, seed=9)),   # 21 long rows + 20 band rows cover a column: 42 * 7 lines
    "n200": ({"n200", "band8", "long5", "large_loop"}, dict(n_kf=200, band=8, n_old_loops=3, loop_rot_deg=20, loop_scale=1.1, seed=10, n_points=60)),
    "band1": ({"band1"}, dict(n_kf=40, band=1, loop_kf=3, seed=11)),
    "band3_nolong": ({"band3", "long0"}, dict(n_kf=24, band=3, n_loop=0, seed=12, meas_noise=0.01)),
    "band8": ({"band8", "long5"}, dict(n_kf=48, band=8, loop_kf=4, n_old_loops=2, seed=13, n_points=20)),
    "one_long": ({"long1"}, dict(n_kf=30, band=0, n_loop=1, loop_kf=1, seed=14, meas_noise=0.005)),
    "fix_scale": ({"fix_scale", "sigma<eps"}, dict(n_kf=30, band=3, fix_scale=True, seed=526)),
    # with the scale fixed the fifth iteration's first trial has rho within rounding of zero: graphs of this size keep one path across the
    # oracle's builds on one seed in twelve.  Under a constant of 2.5e5 in chi2 (an edge between two fixed vertices) every decision is
    # clear and the stagnation rule ends the solve at iteration 3 — on every seed tried
    "fix_scale_b": ({"fix_scale", "sigma<eps", "stagnation", "fixed_pair"}, dict(n_kf=20, band=2, fix_scale=True, seed=700, loop_rot_deg=6, fixed=(0, 1), fixed_pair_edge=True,
                                                                               fixed_pair_offset=500.0)),
    "fix_scale_c": ({"fix_scale", "sigma<eps"}, dict(n_kf=12, band=3, fix_scale=True, seed=105, loop_rot_deg=10, loop_trans=0.5)),
    "free_scale": ({"free_scale"}, dict(n_kf=30, band=3, seed=18, loop_scale=1.05)),
    "several_fixed": ({"several_fixed"}, dict(n_kf=30, band=3, seed=19, fixed=(0, 1, 2, 7), fix_scale_on=(0, 1, 2, 7))),
    "several_fixed_b": ({"several_fixed"}, dict(n_kf=26, band=4, seed=20, fixed=(0, 3, 12, 13), fix_scale_on=(0, 3, 12, 13), n_points=15)),
    "duplicates": ({"duplicates"}, dict(n_kf=30, band=3, seed=21, duplicate_every=3)),
    "duplicates_b": ({"duplicates"}, dict(n_kf=18, band=2, seed=22, duplicate_every=2, n_old_loops=2)),
    "fixed_pair": ({"fixed_pair"}, dict(n_kf=30, band=3, seed=23, fixed=(0, 4), fixed_pair_edge=True)),
    "fixed_pair_b": ({"fixed_pair"}, dict(n_kf=16, band=2, seed=24, fixed=(0, 1), fixed_pair_edge=True)),
    "isolated": ({"isolated"}, dict(n_kf=30, band=3, seed=25, isolated=(5, 17), n_points=20)),
    "isolated_b": ({"isolated"}, dict(n_kf=14, band=2, seed=26, isolated=(3,))),
    "optimum": ({"optimum"}, dict(n_kf=30, band=3, seed=27, start="optimum")),
    "optimum_b": ({"optimum"}, dict(n_kf=12, band=2, seed=29, start="optimum", meas_noise=0.02)),
    "optimum_c": ({"optimum"}, dict(n_kf=20, band=3, seed=38, start="optimum", fix_scale=True, meas_noise=0.01)),
    # a constant of 2.5e5 in chi2 (the edge between the two fixed vertices) under a solve that needs several iterations: each gains less
    # than a thousandth of the whole, and the stagnation rule ends the solve at iteration 3
    "stagnation": ({"stagnation", "fixed_pair"}, dict(n_kf=25, band=4, seed=31, loop_rot_deg=20, loop_scale=0.9, loop_trans=1.0, fixed=(0, 1), fixed_pair_edge=True,
                                                      fixed_pair_offset=500.0)),
    "large_loop": ({"large_loop"}, dict(n_kf=40, band=3, seed=301, loop_rot_deg=20, loop_scale=1.1)),
    "large_loop_b": ({"large_loop"}, dict(n_kf=25, band=4, seed=101, loop_rot_deg=20, loop_scale=0.9, loop_trans=1.0)),
    "near_d": ({"near_d"}, dict(n_kf=9, band=2, seed=32, loop_rot_deg=2.3, loop_trans=0.05, loop_scale=1.0, drift_rot_deg=0.0)),
    "near_d_b": ({"near_d"}, dict(n_kf=12, band=2, seed=33, loop_rot_deg=3.0, loop_trans=0.02, loop_scale=1.01)),
    "near_d_c": ({"near_d"}, dict(n_kf=6, band=1, seed=34, loop_rot_deg=1.2, loop_trans=0.02, fix_scale=True)),
}
CLASSES = ("n2", "n3", "n9", "panel-1", "panel", "panel+1", "lines>256", "n200", "band1", "band3", "band8", "long0", "long1", "long5", "long_span",
           "fix_scale", "free_scale", "several_fixed", "duplicates", "fixed_pair", "isolated", "optimum", "stagnation", "large_loop", "near_d", "sigma<eps")

# Final chi2, GPU against oracle, relative: ten times the largest spread between the two oracle builds over the cases whose LM paths agree.
# test_corpus_selection measures that spread: 1.716e-8, at band3_nolong, where the 1e-9 differences carry ~1e-7 of noise into the Jacobians
# of four iterations (most cases are at 1e-14), and holds the margin between 10 and 10.5 times it — profiles/r17/README.md.  Below CHI2_FLOOR
# a chi2 is rounding noise: seven squared errors of ~1e-10, which is what FP64 leaves of the log of a product of transforms of norm ~10.
CHI2_MARGIN = 1.72e-7
CHI2_FLOOR = 1e-18


@functools.lru_cache(maxsize=None)
def case_problem(name):
    kw = dict(CASES[name][1])
    start = kw.pop("start", None)
    p = make_essential_graph_problem(**kw)
    if start == "optimum":
        p["kfSim3"] = eo.run(p)["kfSim3"]
    return p


@functools.lru_cache(maxsize=None)
def case_oracle(name, flags=eo.DEFAULT_FLAGS):
    return eo.run(case_problem(name), flags)


def builds_agree(name):
    """The two builds of the oracle take the same Levenberg-Marquardt path."""
    a, b = case_oracle(name), case_oracle(name, eo.OTHER_FLAGS)
    return a["stats4"].tolist() == b["stats4"].tolist()


def pinned(name):
    """... and so do the perturbed builds (eo.PERTURBED_FLAGS).  The two builds share one libm and one elimination order, so they can agree on a
    decision that the last bit of acos or of a pivot turns; the GPU has its own of both.  The GPU's path is asserted wherever the two builds
    agree; the seeds are chosen so that every such case is pinned in this sense too (test_corpus_selection)."""
    return builds_agree(name) and all(case_oracle(name, f)["stats4"].tolist() == case_oracle(name)["stats4"].tolist() for f in eo.PERTURBED_FLAGS)


def moved_by_rounding(name):
    """Largest difference of the estimates between the first build and any other."""
    a = case_oracle(name)["kfSim3"]
    return max(np.abs(a - case_oracle(name, f)["kfSim3"]).max() for f in (eo.OTHER_FLAGS,) + eo.PERTURBED_FLAGS)


def problem_bytes(p):
    """A problem as tests/native/essential_graph_adapter_check.cc reads it."""
    return (np.array([len(p["kfSim3"]), len(p["eI"]), len(p["mpPos"])], np.int32).tobytes() + np.ascontiguousarray(p["kfSim3"], np.float64).tobytes() +
            np.ascontiguousarray(p["kfFlags"], np.uint8).tobytes() + np.ascontiguousarray(p["eI"], np.int32).tobytes() + np.ascontiguousarray(p["eJ"], np.int32).tobytes() +
            np.ascontiguousarray(p["eSji"], np.float64).tobytes() + np.ascontiguousarray(p["mpPos"], np.float32).tobytes() + np.ascontiguousarray(p["mpRef"], np.int32).tobytes())
