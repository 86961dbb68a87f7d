"""The corpus of the map-merging pose graph's tests (morb_optimize_essential_graph_merge, the second overload of
Optimizer::OptimizeEssentialGraph): small problems of synth.make_merge_graph_problem, one or more per class, each with the classes it stands
for.  case_problem / case_oracle build and cache; test_merge_graph_cpu.py::test_corpus_selection runs every case through both builds of the
oracle and the perturbed ones and checks that they agree on the Levenberg-Marquardt path of at least half the cases and of at least one of
every class: only those pin the GPU's path.  Most cases carry the reference's constant of chi2 — the edges between two fixed vertices, which
measure a pose itself or mix a corrected pose with a pose before the merge.  Where it is a thousand times the first gain, g2o's stop rule
ends the solve at iteration 3 (`merge`); most small cases end earlier, on ten rejected trials (profiles/r21/README.md)."""
import functools

import numpy as np

import merge_graph_oracle as mo
from essential_graph_cases import CHI2_FLOOR, PANEL   # noqa: F401
from morb_slam_amd.synth import make_merge_graph_problem

# name -> (classes, keyword arguments of the generator)
CASES = {
    # one keyframe per list: the free vertex hangs on the window's, which hangs on the merged map's by the mixed measurement
    "smallest": ({"smallest", "points_each_list"}, dict(n_fixed=1, n_window=1, n_nonfixed=1, overlap=False, band=1, n_old_loops=0, seed=1, n_points=8)),
    # the normal merge shape.  The merged map lies far from the world origin, so the edges among vpFixedKFs, which measure the parent's pose
    # itself, put a constant of 9e5 under chi2: each of three accepted iterations gains less than a thousandth of it
    "merge": ({"merge", "stagnation", "inside", "points_each_list"}, dict(n_fixed=6, n_window=5, n_nonfixed=20, seed=2, n_points=40, origin=(200.0, 0.0, 100.0),
                                                                    corr_trans=5.0, corr_rot_deg=15.0, corr_scale=1.1)),
    "merge_b": ({"merge", "inside"}, dict(n_fixed=6, n_window=5, n_nonfixed=20, seed=3, n_old_loops=2, corr_rot_deg=12.0, corr_scale=0.93, reroot=False)),
    # no edge with an end in vpFixedKFs and none between two window keyframes: chi2 has no constant, and the solve runs four iterations, until
    # ten trials in a row are rejected
    "no_fixed_edge": ({"no_fixed_edge", "inside"}, dict(n_fixed=2, n_window=3, n_nonfixed=14, seed=11, fixed_links=False, weld=False, reroot=False, window_links=False,
                                                         long_loop=True, corr_rot_deg=40.0, corr_trans=8.0, corr_scale=1.5)),
    "no_fixed_edge_b": ({"inside"}, dict(n_fixed=2, n_window=2, n_nonfixed=14, seed=4, fixed_links=False, weld=False, reroot=False, window_links=False,
                                         long_loop=True, corr_rot_deg=3.0, corr_trans=0.3, corr_scale=1.03)),
    "panel_plus": ({"panel+1", "inside"}, dict(n_fixed=3, n_window=3, n_nonfixed=PANEL + 8, seed=6, long_loop=True, n_points=20)),
    "disjoint": ({"disjoint", "points_each_list"}, dict(n_fixed=4, n_window=3, n_nonfixed=9, overlap=False, seed=10, n_points=30)),
    "disjoint_b": ({"disjoint"}, dict(n_fixed=3, n_window=2, n_nonfixed=6, overlap=False, seed=8, band=2, reroot=False)),
    "bad_parent": ({"bad_parent", "inside"}, dict(n_fixed=4, n_window=3, n_nonfixed=12, seed=9, bad=(8,), band=2, n_points=12)),
    "bad_parent_b": ({"bad_parent", "inside"}, dict(n_fixed=3, n_window=3, n_nonfixed=10, seed=10, bad=(1, 6), band=1)),
    "no_edge": ({"no_edge", "inside"}, dict(n_fixed=4, n_window=3, n_nonfixed=12, seed=15, isolated=(7,), n_points=24)),
    "no_edge_b": ({"no_edge", "inside"}, dict(n_fixed=2, n_window=2, n_nonfixed=9, seed=12, isolated=(4, 6), band=2)),
    # the non-fixed list is the window itself: every vertex is fixed, the solve is skipped, the tail still runs
    "no_free": ({"no_free", "inside", "points_each_list"}, dict(n_fixed=3, n_window=4, n_nonfixed=4, seed=13, n_points=16)),
    "no_points": ({"no_points", "inside"}, dict(n_fixed=3, n_window=3, n_nonfixed=8, seed=14, n_points=0)),
}
CLASSES = ("smallest", "merge", "stagnation", "no_fixed_edge", "panel+1", "inside", "disjoint", "bad_parent", "no_edge", "no_free", "points_each_list", "no_points")

# Final chi2, GPU against oracle, relative: ten times the largest spread between the two oracle builds over the cases whose LM paths agree
# (test_merge_graph_cpu.py::test_corpus_selection measures it and holds the margin between 10 and 10.5 times it; profiles/r21/README.md).
# The spread is 6.78e-9, at no_edge_b; under the constant of the fixed-fixed edges most cases are at 1e-13 or below.
CHI2_MARGIN = 6.85e-8


@functools.lru_cache(maxsize=None)
def case_problem(name):
    return make_merge_graph_problem(**CASES[name][1])


@functools.lru_cache(maxsize=None)
def case_oracle(name, flags=mo.DEFAULT_FLAGS):
    return mo.run(case_problem(name), flags)


def builds_agree(name):
    """The two builds of the oracle take the same Levenberg-Marquardt path."""
    return case_oracle(name)["stats4"].tolist() == case_oracle(name, mo.OTHER_FLAGS)["stats4"].tolist()


def pinned(name):
    """... and so do the perturbed builds (essential_graph_cases.pinned says why)."""
    return builds_agree(name) and all(case_oracle(name, f)["stats4"].tolist() == case_oracle(name)["stats4"].tolist() for f in mo.PERTURBED_FLAGS)


def moved_by_rounding(name):
    """Largest difference of a pose or a point between the first build and any other."""
    a = case_oracle(name)
    worst = 0.0
    for f in (mo.OTHER_FLAGS,) + mo.PERTURBED_FLAGS:
        b = case_oracle(name, f)
        for k in mo.POSES + ("mpPos",):
            if len(a[k]):
                worst = max(worst, float(np.abs(pose_diff(a[k], b[k]) if k != "mpPos" else a[k] - b[k]).max()))
    return worst


def pose_diff(a, b):
    """a - b for [n, 7] poses, with b's quaternions taken on a's side of the double cover."""
    b = b.copy()
    flip = (a[:, :4] * b[:, :4]).sum(1) < 0
    b[flip, :4] = -b[flip, :4]
    return a - b


def problem_bytes(p):
    """A problem as tests/native/merge_graph_adapter_check.cc reads it."""
    return (np.array([len(p["kfLists"]), len(p["cI"]), len(p["mpPos"])], np.int32).tobytes() + np.ascontiguousarray(p["kfLists"], np.uint8).tobytes() +
            b"".join(np.ascontiguousarray(p[k], np.float32).tobytes() for k in mo.POSES) + np.ascontiguousarray(p["cI"], np.int32).tobytes() +
            np.ascontiguousarray(p["cJ"], np.int32).tobytes() + np.ascontiguousarray(p["mpPos"], np.float32).tobytes() + np.ascontiguousarray(p["mpRef"], np.int32).tobytes())
