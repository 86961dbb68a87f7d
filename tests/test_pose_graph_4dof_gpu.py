"""Optimizer::OptimizeEssentialGraph4DoF on the GPU (morb_optimize_essential_graph_4dof, Optimizer.OptimizeEssentialGraph4DoF) against the
CPU oracle of tests/native/pose_graph_4dof_oracle.cc over the corpus of tests/pose_graph_4dof_cases.py; repeatability, workspace reuse
(also across the two pose graphs that share the handle's block), and the refused calls."""
import numpy as np
import pytest

import essential_graph_cases as eg_cases
import pose_graph_4dof_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, points=True):
    return opt.OptimizeEssentialGraph4DoF(p["kfPose"], p["kfBody"], p["kfFixed"], p["Tcb12"], p["eI"], p["eJ"], p["eTij"], p["mpPos"] if points else None,
                                          p["mpRef"] if points else None, p["kfScw"] if points else None)


def _call7(opt, p):
    return opt.OptimizeEssentialGraph(p["kfSim3"], p["kfFlags"], p["eI"], p["eJ"], p["eSji"], p["mpPos"], p["mpRef"])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_matches_the_oracle(opt, name):
    """Poses (all 12 entries) and corrected points within 1e-4 of the oracle; the final chi2 within cases.CHI2_MARGIN (ten times the spread
    between the two oracle builds, measured on the CPU) relative, above the floor where a chi2 is rounding noise; vertices in the system and
    envelope blocks equal; (iterations, trials) equal on every case; fixed vertices, vertices without an edge and points without a
    reference keep their bytes."""
    p, want = cases.case_problem(name), cases.case_oracle(name)
    P, mp, stats, chi2 = _call(opt, p)
    rel = abs(chi2[1] - want["chi2"][1]) / max(want["chi2"][1], cases.CHI2_FLOOR)
    print(name, "edges", len(p["eI"]), "stats4", stats.tolist(), "oracle", want["stats4"].tolist(), "poses", np.abs(P - want["kfPose"]).max(),
          "points", np.abs(mp - want["mpPos"]).max() if len(mp) else 0.0, "chi2", chi2.tolist(), "oracle", want["chi2"].tolist(), "relative", rel)
    assert stats.tolist() == want["stats4"].tolist()
    assert np.abs(P - want["kfPose"]).max() <= 1e-4
    if len(mp):
        assert np.abs(mp - want["mpPos"]).max() <= 1e-4
    assert abs(chi2[0] - want["chi2"][0]) <= cases.CHI2_MARGIN * want["chi2"][0] + cases.CHI2_FLOOR
    assert abs(chi2[1] - want["chi2"][1]) <= cases.CHI2_MARGIN * want["chi2"][1] + cases.CHI2_FLOOR
    still = (p["kfFixed"] != 0) | ~np.isin(np.arange(len(P)), np.concatenate([p["eI"], p["eJ"]]))
    assert still.any() and P[still].tobytes() == p["kfPose"][still].tobytes()
    assert mp[p["mpRef"] < 0].tobytes() == p["mpPos"][p["mpRef"] < 0].tobytes()
    if "optimum" in cases.CASES[name][0]:   # every trial rejected: no byte changes
        assert P.tobytes() == p["kfPose"].tobytes() and chi2[0] == chi2[1]


def test_two_runs_give_identical_bytes(opt):
    for name in ("n200", "two_passes", "duplicates", "stage_plus"):
        a, b = _call(opt, cases.case_problem(name)), _call(opt, cases.case_problem(name))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), name


def test_a_reused_workspace_gives_the_bytes_of_a_fresh_one():
    """The handle's block is carved anew at every call: behind a larger graph a call finds other offsets and whatever the last one left (a
    factor, Jacobians of vertices that are now fixed, LM words), behind a smaller one the block grows."""
    from morb_slam_amd import Optimizer
    order = ("band8", "n9", "n200", "several_fixed", "n2", "two_passes")
    shared = Optimizer(0)
    try:
        for name in order:
            got = _call(shared, cases.case_problem(name))
            fresh = Optimizer(0)
            try:
                want = _call(fresh, cases.case_problem(name))
            finally:
                fresh.close()
            for x, y in zip(got, want):
                assert x.tobytes() == y.tobytes(), name
    finally:
        shared.close()


def test_interleaved_with_the_sim3_pose_graph_on_one_handle():
    """morb_optimize_essential_graph and the 4-DoF call carve the same block of the handle: interleaved on one handle, each gives the bytes
    it gives on a handle of its own."""
    from morb_slam_amd import Optimizer
    order = (("4", "band8"), ("7", "band8"), ("4", "n200"), ("7", "n9"), ("4", "n9"), ("7", "n200"), ("4", "stage"))
    shared = Optimizer(0)
    try:
        for kind, name in order:
            fresh = Optimizer(0)
            try:
                if kind == "4":
                    got, want = _call(shared, cases.case_problem(name)), _call(fresh, cases.case_problem(name))
                else:
                    got, want = _call7(shared, eg_cases.case_problem(name)), _call7(fresh, eg_cases.case_problem(name))
            finally:
                fresh.close()
            for x, y in zip(got, want):
                assert x.tobytes() == y.tobytes(), (kind, name)
    finally:
        shared.close()


def test_no_points(opt):
    p = cases.case_problem("n9")
    P, mp, stats, chi2 = _call(opt, p, points=False)
    full = _call(opt, p)
    assert len(mp) == 0 and P.tobytes() == full[0].tobytes() and stats.tolist() == full[2].tolist() and chi2.tobytes() == full[3].tobytes()


def test_any_non_zero_byte_fixes_a_vertex(opt):
    p = dict(cases.case_problem("several_fixed"))
    want = _call(opt, p)
    p["kfFixed"] = (p["kfFixed"] * np.array([2, 255, 1, 128] * 8, np.uint8)[:len(p["kfFixed"])]).astype(np.uint8)
    assert sorted(set(p["kfFixed"].tolist())) == [0, 1, 2, 128, 255]
    for x, y in zip(_call(opt, p), want):
        assert x.tobytes() == y.tobytes()


def test_wrapper_gives_the_bytes_of_the_c_entry(opt):
    from morb_slam_amd.capi import MORB_OK, lib, ptr
    p = cases.case_problem("band8")
    P, B, fx = np.ascontiguousarray(p["kfPose"], np.float64).copy(), np.ascontiguousarray(p["kfBody"], np.float64), np.ascontiguousarray(p["kfFixed"], np.uint8)
    mp, ref, scw = p["mpPos"].copy(), p["mpRef"], np.ascontiguousarray(p["kfScw"], np.float64)
    stats, chi2 = np.zeros(4, np.int32), np.zeros(2)
    assert lib().morb_optimize_essential_graph_4dof(opt._h, len(P), ptr(P), ptr(B), ptr(fx), ptr(p["Tcb12"]), len(p["eI"]), ptr(p["eI"]), ptr(p["eJ"]), ptr(p["eTij"]),
                                                    len(mp), ptr(mp), ptr(ref), ptr(scw), ptr(stats), ptr(chi2)) == MORB_OK
    for x, y in zip((P, mp, stats, chi2), _call(opt, p)):
        assert x.tobytes() == y.tobytes()


def test_refused_calls(opt):
    from morb_slam_amd.capi import ERR_CAPACITY, ERR_INVALID, MORB_OK, lib, ptr
    L = lib()
    p = cases.case_problem("n9")
    base = dict(P=np.ascontiguousarray(p["kfPose"], np.float64).copy(), B=np.ascontiguousarray(p["kfBody"], np.float64).copy(), fx=p["kfFixed"].copy(),
                tcb=p["Tcb12"].copy(), eI=p["eI"].copy(), eJ=p["eJ"].copy(), M=p["eTij"].copy(), mp=p["mpPos"].copy(), ref=p["mpRef"].copy(),
                scw=np.ascontiguousarray(p["kfScw"], np.float64).copy())
    stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)

    def call(h=opt._h, **kw):
        a = {k: (v.copy() if v is not None else None) for k, v in {**base, **kw}.items()}
        q = lambda x: ptr(x) if x is not None else None
        keep = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        rc = L.morb_optimize_essential_graph_4dof(h, len(a["fx"]), q(a["P"]), q(a["B"]), q(a["fx"]), q(a["tcb"]), len(a["eI"]) if a["eI"] is not None else 1,
                                                  q(a["eI"]), q(a["eJ"]), q(a["M"]), len(a["ref"]) if a["ref"] is not None else 3, q(a["mp"]), q(a["ref"]),
                                                  q(a["scw"]), ptr(stats), ptr(chi2))
        for k in a:
            assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k   # nothing written
        return rc

    for kw in (dict(h=None), dict(P=None), dict(B=None), dict(tcb=None), dict(eI=None), dict(eJ=None), dict(M=None), dict(mp=None), dict(ref=None), dict(scw=None)):
        assert call(**kw) == ERR_INVALID, kw
    n = len(base["fx"])
    assert L.morb_optimize_essential_graph_4dof(opt._h, n, ptr(base["P"].copy()), ptr(base["B"]), None, ptr(base["tcb"]), len(base["eI"]), ptr(base["eI"]), ptr(base["eJ"]),
                                                ptr(base["M"]), 0, None, None, None, ptr(stats), ptr(chi2)) == ERR_INVALID   # kfFixed
    bad = base["eI"].copy(); bad[-1] = n
    assert call(eI=bad) == ERR_INVALID
    bad = base["eJ"].copy(); bad[0] = -1
    assert call(eJ=bad) == ERR_INVALID
    bad = base["eJ"].copy(); bad[3] = base["eI"][3]
    assert call(eJ=bad) == ERR_INVALID                                   # eI == eJ
    for key, idx, v in (("P", (4, 2), np.nan), ("P", (0, 11), np.inf), ("B", (3, 5), np.nan), ("B", (1, 10), -np.inf), ("M", (1, 7), np.nan), ("tcb", (4,), np.nan),
                        ("scw", (2, 1), np.inf), ("scw", (2, 7), 0.0), ("scw", (5, 7), -1.0)):
        bad = base[key].copy(); bad[idx] = v
        assert call(**{key: bad}) == ERR_INVALID, (key, idx, v)
    bad = base["ref"].copy(); bad[0] = n
    assert call(ref=bad) == ERR_INVALID
    assert stats.tolist() == [-7] * 4 and chi2.tolist() == [-7.0] * 2
    # the envelope of a star around the first free vertex: n (n + 1) / 2 blocks, beyond the 2^22 a handle may grow to; before any launch
    n = 3000
    I12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.0])
    P = np.tile(I12, (n, 1)); fx = np.zeros(n, np.uint8); fx[0] = 1
    eI = np.arange(1, n, dtype=np.int32); eJ = np.zeros(n - 1, np.int32); eJ[1:] = 1
    M = np.tile(I12, (n - 1, 1))
    assert call(P=P, B=P.copy(), fx=fx, eI=eI, eJ=eJ, M=M, mp=None, ref=np.zeros(0, np.int32), scw=None) == ERR_CAPACITY
    assert stats.tolist() == [-7] * 4
    # no free vertex on any edge: MORB_OK, zero stats, nothing written
    fx = base["fx"].copy(); fx[:] = 1
    assert call(fx=fx) == MORB_OK and stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
    stats[:] = -7; chi2[:] = -7.0   # ... and a map without an edge at all is that case too
    assert L.morb_optimize_essential_graph_4dof(opt._h, 1, ptr(base["P"][:1].copy()), ptr(base["B"][:1].copy()), ptr(base["fx"][:1].copy()), ptr(base["tcb"]), 0, None, None,
                                                None, 0, None, None, None, ptr(stats), ptr(chi2)) == MORB_OK
    assert stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
