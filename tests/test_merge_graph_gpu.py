"""The second overload of Optimizer::OptimizeEssentialGraph on the GPU (morb_optimize_essential_graph_merge,
Optimizer.OptimizeEssentialGraphMerge) against the CPU oracle of tests/native/merge_graph_oracle.cc over the corpus of
tests/merge_graph_cases.py; the stagnation ending, repeatability, workspace reuse across sizes and across the first overload, the wrapper,
and the refused calls."""
import numpy as np
import pytest

import essential_graph_cases as eg_cases
import merge_graph_cases as cases
import merge_graph_oracle as mo

pytestmark = pytest.mark.gpu
OUT = mo.POSES + ("mpPos", "cKept", "stats4", "chi2")


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, points=True):
    return opt.OptimizeEssentialGraphMerge(p["kfLists"], *[p[k] for k in mo.POSES], p["cI"], p["cJ"], p["mpPos"] if points else None, p["mpRef"] if points else None)


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in OUT)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_matches_the_oracle(opt, name):
    """Tcw / Twc (quaternion and translation) and corrected points within 1e-4 of the oracle; kept-edge flags, vertices in the system and
    envelope blocks equal; (iterations, trials) equal wherever the two oracle builds agree; both chi2 within cases.CHI2_MARGIN (ten times
    the spread between the two oracle builds, measured on the CPU) relative, plus the floor below which a chi2 is rounding noise.  The
    BefMerge outputs carry the entry bytes of Tcw / Twc exactly for the vertices of vpNonFixedKFs and their own bytes otherwise; Tcw / Twc
    of the other vertices and points with an unflagged or -1 reference keep their bytes."""
    p, want = cases.case_problem(name), cases.case_oracle(name)
    got = _call(opt, p)
    pinned = cases.builds_agree(name)
    worst = {k: float(np.abs(cases.pose_diff(got[k], want[k])).max()) for k in ("kfTcw", "kfTwc")}
    worst["mpPos"] = float(np.abs(got["mpPos"] - want["mpPos"]).max()) if len(p["mpPos"]) else 0.0
    print(name, "candidates", len(p["cI"]), "kept", int(got["cKept"].sum()), "stats4", got["stats4"].tolist(), "oracle", want["stats4"].tolist(),
          "pinned" if pinned else "NOT pinned", worst, "chi2", got["chi2"].tolist(), "oracle", want["chi2"].tolist())
    assert got["cKept"].tolist() == want["cKept"].tolist()
    assert got["stats4"][2:].tolist() == want["stats4"][2:].tolist()
    if pinned:
        assert got["stats4"][:2].tolist() == want["stats4"][:2].tolist()
    assert max(worst.values()) <= 1e-4
    for k in range(2):
        assert abs(got["chi2"][k] - want["chi2"][k]) <= cases.CHI2_MARGIN * want["chi2"][k] + cases.CHI2_FLOOR
    lists = p["kfLists"]
    tail = (lists & 4) != 0
    for k, src in (("kfTcwBefMerge", "kfTcw"), ("kfTwcBefMerge", "kfTwc")):
        assert got[k][tail].tobytes() == p[src][tail].tobytes() and got[k][~tail].tobytes() == p[k][~tail].tobytes()
        assert got[src][~tail].tobytes() == p[src][~tail].tobytes()
    if len(p["mpPos"]):
        ref = p["mpRef"]
        stays = (ref < 0) | (lists[np.maximum(ref, 0)] == 1)
        assert got["mpPos"][stays].tobytes() == p["mpPos"][stays].tobytes()


def test_stagnation_ends_at_iteration_three_and_still_moves_the_map(opt):
    """The normal merge shape: the constant of the fixed-fixed edges ends the solve by g2o's stop rule at iteration 3, and the free
    keyframes next to the window have moved by far more than 1e-3 by then."""
    p = cases.case_problem("merge")
    got = _call(opt, p)
    assert got["stats4"][:2].tolist() == [3, 3] and got["chi2"][0] - got["chi2"][1] < 1e-3 * got["chi2"][1]
    window = np.array(p["window"])
    near = np.arange(window.min() - 3, window.min())   # the last free keyframes of the chain
    assert (p["kfLists"][near] == 4).all()
    assert np.abs(got["kfTcw"][near, 4:] - p["kfTcw"][near, 4:]).max(axis=1).min() > 1e-3


def test_two_runs_give_identical_bytes(opt):
    for name in ("merge", "panel_plus", "no_free"):
        a, b = _call(opt, cases.case_problem(name)), _call(opt, cases.case_problem(name))
        assert _same_bytes(a, b), name


def test_a_reused_workspace_gives_the_bytes_of_a_fresh_one():
    """The handle's block is carved anew at every call, and the first overload carves the same block: behind a larger graph, a smaller one, a
    call without a solve and a call of morb_optimize_essential_graph every merge call gives the bytes of a fresh handle — and so does the
    first overload behind a merge call."""
    from morb_slam_amd import Optimizer
    order = ("merge", "smallest", "panel_plus", "eg:n9", "no_free", "disjoint", "eg:band8", "no_fixed_edge")

    def run(o, name):
        if name.startswith("eg:"):
            q = eg_cases.case_problem(name[3:])
            return dict(zip("abcd", o.OptimizeEssentialGraph(q["kfSim3"], q["kfFlags"], q["eI"], q["eJ"], q["eSji"], q["mpPos"], q["mpRef"])))
        return _call(o, cases.case_problem(name))

    shared = Optimizer(0)
    try:
        for name in order:
            got = run(shared, name)
            fresh = Optimizer(0)
            try:
                want = run(fresh, name)
            finally:
                fresh.close()
            assert all(got[k].tobytes() == want[k].tobytes() for k in want), name
    finally:
        shared.close()


def test_no_points(opt):
    p = cases.case_problem("merge")
    got, full = _call(opt, p, points=False), _call(opt, p)
    assert len(got["mpPos"]) == 0 and all(got[k].tobytes() == full[k].tobytes() for k in OUT if k != "mpPos")


def test_wrapper_gives_the_bytes_of_the_c_entry(opt):
    from morb_slam_amd.capi import MORB_OK, lib, ptr
    p = cases.case_problem("disjoint")
    poses = [p[k].copy() for k in mo.POSES]
    mp, kept, stats, chi2 = p["mpPos"].copy(), np.zeros(len(p["cI"]), np.uint8), np.zeros(4, np.int32), np.zeros(2)
    assert lib().morb_optimize_essential_graph_merge(opt._h, len(p["kfLists"]), ptr(p["kfLists"]), *[ptr(a) for a in poses], len(p["cI"]), ptr(p["cI"]), ptr(p["cJ"]),
                                                     ptr(kept), len(mp), ptr(mp), ptr(p["mpRef"]), ptr(stats), ptr(chi2)) == MORB_OK
    got = _call(opt, p)
    for k, a in zip(OUT, poses + [mp, kept, stats, chi2]):
        assert a.tobytes() == got[k].tobytes(), k


def test_refused_calls(opt):
    from morb_slam_amd.capi import ERR_CAPACITY, ERR_INVALID, MORB_OK, lib, ptr
    L = lib()
    p = cases.case_problem("bad_parent")
    base = dict(lists=p["kfLists"].copy(), Tcw=p["kfTcw"].copy(), Twc=p["kfTwc"].copy(), TcwBef=p["kfTcwBefMerge"].copy(), TwcBef=p["kfTwcBefMerge"].copy(),
                cI=p["cI"].copy(), cJ=p["cJ"].copy(), kept=np.full(len(p["cI"]), 9, np.uint8), mp=p["mpPos"].copy(), ref=p["mpRef"].copy())
    stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)

    def call(h=opt._h, **kw):
        a = {k: (v.copy() if v is not None else None) for k, v in {**base, **kw}.items()}
        q = lambda x: ptr(x) if x is not None else None
        keep = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        rc = L.morb_optimize_essential_graph_merge(h, len(a["lists"]) if a["lists"] is not None else 3, q(a["lists"]), q(a["Tcw"]), q(a["Twc"]), q(a["TcwBef"]), q(a["TwcBef"]),
                                                   len(a["cI"]) if a["cI"] is not None else 1, q(a["cI"]), q(a["cJ"]), q(a["kept"]),
                                                   len(a["ref"]) if a["ref"] is not None else 3, q(a["mp"]), q(a["ref"]), ptr(stats), ptr(chi2))
        if rc != MORB_OK:
            for k in a:
                assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k   # nothing written
        return rc

    for k in ("h", "lists", "Tcw", "Twc", "TcwBef", "TwcBef", "cI", "cJ", "kept", "mp", "ref"):
        assert call(**{k: None}) == ERR_INVALID, k
    bad = base["cI"].copy(); bad[-1] = len(base["lists"])
    assert call(cI=bad) == ERR_INVALID
    bad = base["cJ"].copy(); bad[0] = -1
    assert call(cJ=bad) == ERR_INVALID
    bad = base["cJ"].copy(); bad[3] = base["cI"][3]
    assert call(cJ=bad) == ERR_INVALID                                   # cI == cJ
    for name in ("Tcw", "Twc"):
        for k, v in ((2, np.nan), (5, np.inf)):
            bad = base[name].copy(); bad[4, k] = v
            assert call(**{name: bad}) == ERR_INVALID, (name, k, v)
    window = int(np.flatnonzero(base["lists"] & 2)[0]); other = int(np.flatnonzero(base["lists"] == 4)[0])
    bad = base["TcwBef"].copy(); bad[window, 1] = np.nan
    assert call(TcwBef=bad) == ERR_INVALID                               # read for a window keyframe ...
    bad = base["Tcw"].copy(); bad[2, :4] = 0
    assert call(Tcw=bad) == ERR_INVALID                                  # a quaternion that cannot be normalised
    for mask in (0, 3, 5, 7, 8):
        bad = base["lists"].copy(); bad[other] = mask
        assert call(lists=bad) == ERR_INVALID, mask
    bad = base["ref"].copy(); bad[0] = len(base["lists"])
    assert call(ref=bad) == ERR_INVALID
    assert stats.tolist() == [-7] * 4 and chi2.tolist() == [-7.0] * 2
    # the envelope of a star around the first free vertex: n (n + 1) / 2 blocks, beyond the 2^22 a handle may grow to; before any launch
    n = 3000
    ident = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
    lists = np.full(n, 4, np.uint8); lists[0] = 2
    cI = np.arange(1, n, dtype=np.int32); cJ = np.zeros(n - 1, np.int32); cJ[1:] = 1
    assert call(lists=lists, Tcw=ident, Twc=ident, TcwBef=ident, TwcBef=ident, cI=cI, cJ=cJ, kept=np.full(n - 1, 9, np.uint8), mp=None, ref=np.zeros(0, np.int32)) == ERR_CAPACITY
    assert stats.tolist() == [-7] * 4
    # ... and not read elsewhere: a non-finite mTcwBefMerge of a keyframe outside the window passes through
    odd = base["TcwBef"].copy(); odd[other, 1] = np.nan
    assert call(TcwBef=odd) == MORB_OK and stats[0] > 0
    # no candidate at all: MORB_OK, zero stats, the tail still runs
    stats[:] = -7; chi2[:] = -7.0
    poses = [base[k].copy() for k in ("Tcw", "Twc", "TcwBef", "TwcBef")]
    assert L.morb_optimize_essential_graph_merge(opt._h, len(base["lists"]), ptr(base["lists"]), *[ptr(a) for a in poses], 0, None, None, None, 0, None, None,
                                                 ptr(stats), ptr(chi2)) == MORB_OK
    assert stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
    tail = (base["lists"] & 4) != 0
    assert poses[2][tail].tobytes() == base["Tcw"][tail].tobytes() and poses[3][tail].tobytes() == base["Twc"][tail].tobytes()
    assert np.abs(cases.pose_diff(poses[0], base["Tcw"])).max() <= 1e-6 * max(1.0, np.abs(base["Tcw"]).max())
