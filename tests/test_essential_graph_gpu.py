"""Optimizer::OptimizeEssentialGraph on the GPU (morb_optimize_essential_graph, Optimizer.OptimizeEssentialGraph) against the CPU oracle of
tests/native/essential_graph_oracle.cc over the corpus of tests/essential_graph_cases.py; repeatability, workspace reuse, the refused
calls, and the device library's acos / log against the host libm."""
import math

import numpy as np
import pytest

import essential_graph_cases as cases
import essential_graph_oracle as eo
from morb_slam_amd.synth import make_essential_graph_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, points=True):
    return opt.OptimizeEssentialGraph(p["kfSim3"], p["kfFlags"], p["eI"], p["eJ"], p["eSji"], p["mpPos"] if points else None, p["mpRef"] if points else None)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_matches_the_oracle(opt, name):
    """Vertex estimates and corrected points within 1e-4 of the oracle; the final chi2 within cases.CHI2_MARGIN (ten times the spread between
    the two oracle builds, measured on the CPU) relative, above the floor where a chi2 is rounding noise; vertices in the system and envelope
    blocks equal; (iterations, trials) equal wherever the two oracle builds agree on them; fixed vertices, vertices without an edge and
    points without a reference keep their bytes."""
    p, want = cases.case_problem(name), cases.case_oracle(name)
    S, mp, stats, chi2 = _call(opt, p)
    pinned = cases.builds_agree(name)
    rel = abs(chi2[1] - want["chi2"][1]) / max(want["chi2"][1], cases.CHI2_FLOOR)
    print(name, "edges", len(p["eI"]), "stats4", stats.tolist(), "oracle", want["stats4"].tolist(), "pinned" if pinned else "NOT pinned", "vertices", np.abs(S - want["kfSim3"]).max(),
          "points", np.abs(mp - want["mpPos"]).max() if len(mp) else 0.0, "chi2", chi2.tolist(), "oracle", want["chi2"].tolist(), "relative", rel)
    assert stats[2:].tolist() == want["stats4"][2:].tolist()
    if pinned:
        assert stats[:2].tolist() == want["stats4"][:2].tolist()
    assert np.abs(S - want["kfSim3"]).max() <= 1e-4
    if len(mp):
        assert np.abs(mp - want["mpPos"]).max() <= 1e-4
    assert abs(chi2[0] - want["chi2"][0]) <= cases.CHI2_MARGIN * want["chi2"][0] + cases.CHI2_FLOOR
    assert abs(chi2[1] - want["chi2"][1]) <= cases.CHI2_MARGIN * want["chi2"][1] + cases.CHI2_FLOOR
    still = ((p["kfFlags"] & 1) != 0) | ~np.isin(np.arange(len(S)), np.concatenate([p["eI"], p["eJ"]]))
    assert S[still].tobytes() == p["kfSim3"][still].tobytes()
    assert mp[p["mpRef"] < 0].tobytes() == p["mpPos"][p["mpRef"] < 0].tobytes()


def test_two_runs_give_identical_bytes(opt):
    for name in ("n200", "two_passes", "duplicates"):
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


def test_no_points(opt):
    p = cases.case_problem("n9")
    S, mp, stats, chi2 = _call(opt, p, points=False)
    full = _call(opt, p)
    assert len(mp) == 0 and S.tobytes() == full[0].tobytes() and stats.tolist() == full[2].tolist() and chi2.tobytes() == full[3].tobytes()


def test_wrapper_gives_the_bytes_of_the_c_entry(opt):
    from morb_slam_amd.capi import MORB_OK, lib, ptr
    p = cases.case_problem("band8")
    S, fl = np.ascontiguousarray(p["kfSim3"], np.float64).copy(), np.ascontiguousarray(p["kfFlags"], np.uint8)
    mp, ref = p["mpPos"].copy(), p["mpRef"]
    stats, chi2 = np.zeros(4, np.int32), np.zeros(2)
    assert lib().morb_optimize_essential_graph(opt._h, len(S), ptr(S), ptr(fl), len(p["eI"]), ptr(p["eI"]), ptr(p["eJ"]), ptr(p["eSji"]), len(mp), ptr(mp), ptr(ref),
                                               ptr(stats), ptr(chi2)) == MORB_OK
    for x, y in zip((S, mp, stats, chi2), _call(opt, p)):
        assert x.tobytes() == y.tobytes()


def test_refused_calls(opt):
    from morb_slam_amd.capi import ERR_CAPACITY, ERR_INVALID, MORB_OK, lib, ptr
    L = lib()
    p = cases.case_problem("n9")
    base = dict(S=np.ascontiguousarray(p["kfSim3"], np.float64).copy(), fl=p["kfFlags"].copy(), eI=p["eI"].copy(), eJ=p["eJ"].copy(), M=p["eSji"].copy(),
                mp=p["mpPos"].copy(), ref=p["mpRef"].copy())
    stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)

    def call(h=opt._h, **kw):
        a = {k: (v.copy() if v is not None else None) for k, v in {**base, **kw}.items()}
        q = lambda x: ptr(x) if x is not None else None
        keep = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        rc = L.morb_optimize_essential_graph(h, len(a["fl"]), q(a["S"]), q(a["fl"]), len(a["eI"]) if a["eI"] is not None else 1, q(a["eI"]), q(a["eJ"]), q(a["M"]),
                                             len(a["ref"]) if a["ref"] is not None else 3, q(a["mp"]), q(a["ref"]), ptr(stats), ptr(chi2))
        for k in a:
            assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k   # nothing written
        return rc

    for kw in (dict(h=None), dict(S=None), dict(fl=None), dict(eI=None), dict(eJ=None), dict(M=None), dict(mp=None), dict(ref=None)):
        if "fl" in kw:
            continue   # (its length gives nKF here)
        assert call(**kw) == ERR_INVALID, kw
    bad = base["eI"].copy(); bad[-1] = len(base["fl"])
    assert call(eI=bad) == ERR_INVALID
    bad = base["eJ"].copy(); bad[0] = -1
    assert call(eJ=bad) == ERR_INVALID
    bad = base["eJ"].copy(); bad[3] = base["eI"][3]
    assert call(eJ=bad) == ERR_INVALID                                   # eI == eJ
    for k, v in ((2, np.nan), (5, np.inf), (7, 0.0), (7, -1.0)):
        bad = base["S"].copy(); bad[4, k] = v
        assert call(S=bad) == ERR_INVALID, (k, v)
    bad = base["M"].copy(); bad[1, 7] = 0.0
    assert call(M=bad) == ERR_INVALID
    bad = base["ref"].copy(); bad[0] = len(base["fl"])
    assert call(ref=bad) == ERR_INVALID
    assert stats.tolist() == [-7] * 4 and chi2.tolist() == [-7.0] * 2
    # the envelope of a star around the first free vertex: n (n + 1) / 2 blocks, beyond the 2^22 a handle may grow to; before any launch
    n = 3000
    S = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1)); fl = np.zeros(n, np.uint8); fl[0] = 1
    eI = np.arange(1, n, dtype=np.int32); eJ = np.zeros(n - 1, np.int32); eJ[1:] = 1
    M = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n - 1, 1))
    assert call(S=S, fl=fl, eI=eI, eJ=eJ, M=M, mp=None, ref=np.zeros(0, np.int32)) == ERR_CAPACITY
    assert stats.tolist() == [-7] * 4
    # no free vertex has an edge: MORB_OK, zero stats, nothing written
    fl = base["fl"].copy(); fl[:] = 1
    assert call(fl=fl) == MORB_OK and stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
    stats[:] = -7; chi2[:] = -7.0   # ... and a map without an edge at all is that case too
    assert L.morb_optimize_essential_graph(opt._h, 1, ptr(base["S"][:1].copy()), ptr(base["fl"][:1].copy()), 0, None, None, None, 0, None, None, ptr(stats), ptr(chi2)) == MORB_OK
    assert stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]


def _ulp(got, want):
    return max(abs(g - w) / math.ulp(w) if w != 0 else abs(g) / 5e-324 for g, w in zip(got.tolist(), want))


def test_device_acos_and_log_against_the_host_libm(opt):
    """Sim3::log calls acos(d) for d in (-1, 1 - 1e-5] and log(s); the kernels take the device library's.  Against the host libm (math.acos,
    math.log) on 40 000 arguments each — uniform, and crowded towards both ends of acos' interval — the OpenCL full-profile bounds the
    device library is built to (acos 4 ulp, log 3 ulp) plus the host's own ulp: 5 and 4.  profiles/r17/README.md records what was seen."""
    rng = np.random.default_rng(7)
    d = np.concatenate([rng.uniform(-1, 1 - 1e-5, 20000), 1 - 1e-5 - 10 ** rng.uniform(-9, -1, 10000), -1 + 10 ** rng.uniform(-12, -1, 10000), [1 - 1e-5, 0.0, -0.5, 0.5]])
    d = d[(d > -1) & (d <= 1 - 1e-5)]
    s = np.concatenate([rng.uniform(0.5, 2.0, len(d) - 5), [0.5, 1.0, 2.0, 1 + 1e-9, 1 - 1e-9]])
    a, l = opt.Sim3LogLibm(d, s)
    ua, ul = _ulp(a, [math.acos(x) for x in d.tolist()]), _ulp(l, [math.log(x) for x in s.tolist()])
    print("largest difference from the host libm: acos", ua, "ulp, log", ul, "ulp")
    assert ua <= 5 and ul <= 4
