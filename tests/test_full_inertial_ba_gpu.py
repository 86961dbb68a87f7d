"""FullInertialBA on the GPU (morb_full_inertial_ba*, Optimizer.FullInertialBA) against the CPU oracle of
tests/native/full_inertial_ba_oracle.cc over the corpus of tests/full_inertial_ba_cases.py; workspace reuse; the stop flag; the refused
calls and the two capacity refusals."""
import threading

import numpy as np
import pytest

import full_inertial_ba_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, pre, its, stop_flag=None):
    rig = p["rig28"] is not None
    return opt.FullInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"], pre,
                              p["cam"], p["Tbc12"], its=its, init=p["init"], prior_g=p["priorG"], prior_a=p["priorA"], bias6=p["bias6"],
                              stop_flag=stop_flag, rig=p["rig28"] if rig else None, eRight=p["eRight"] if rig else None)


@pytest.mark.parametrize("case", cases.KEPT, ids=cases.case_id)
def test_matches_the_oracle(opt, case):
    """Same LM path and system (stats4); states and bias6 within 1e-4, points within 1e-4 relative to max(1, |X|); chi2 within ten times the
    oracle builds' spread (floor 1e-6); kinds 1 / 2 keep every byte, kind 3 its velocity / bias floats, keyframes and points without an edge
    everything; with bInit every kind-0 keyframe holds the shared biases; a second call is bit-identical."""
    (p, pre), want = cases.scene(case), cases.case_oracle(case)
    kf, mp, b6, stats, chi2 = _call(opt, p, pre, case[2])
    kind, kf0, mp0 = p["kfKind"], np.ascontiguousarray(p["kfState"], np.float32), np.ascontiguousarray(p["mpPos"], np.float32)
    dk = np.abs(kf.astype(np.float64) - want["kfState"]).max()
    db = np.abs(b6.astype(np.float64) - want["bias6"]).max()
    dp = (np.abs(mp - want["mpPos"]).max(1) / np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).max()
    dc = (np.abs(chi2 - want["chi2"]) / np.maximum(1.0, np.abs(want["chi2"]))).max()
    print(case[0], "edges", len(p["eKF"]), "stats4", stats.tolist(), "oracle", want["stats4"].tolist(), "states", dk, "bias6", db, "points", dp,
          "chi2", chi2.tolist(), "rel", dc)
    assert stats.tolist() == want["stats4"].tolist()
    assert dk <= 1e-4 and db <= 1e-4 and dp <= 1e-4
    assert dc <= max(cases.CHI2_MARGIN, cases.CHI2_FLOOR)
    fixed = (kind == 1) | (kind == 2)
    assert kf[fixed].tobytes() == kf0[fixed].tobytes()
    assert kf[kind == 3][:, 12:].tobytes() == kf0[kind == 3][:, 12:].tobytes()
    seen = np.zeros(len(mp), bool); seen[p["eMP"]] = True
    assert mp[~seen].tobytes() == mp0[~seen].tobytes()
    if p["init"]:
        assert (kf[kind == 0][:, 15:] == b6[None, :]).all()
    else:
        assert b6.tobytes() == np.ascontiguousarray(p["bias6"], np.float32).tobytes()
    again = _call(opt, p, pre, case[2])
    for x, y in zip((kf, mp, b6, stats, chi2), again):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("case", cases.FREE_PATH + cases.LONE, ids=cases.case_id)
def test_call_site_configuration(opt, case):
    """Nothing fixed, as LoopClosing and LocalMapping call it, over 7 and 100 iterations, and the single keyframe standing alone.  The
    states drift along the gauge, which lambda = 1e-5 alone holds (tests/full_inertial_ba_cases.py), so the comparison is gauge-invariant:
    chi2 starts where the oracle's does and falls; the chi2 reported is the chi2 the oracle finds at the state returned (ten times the
    oracle's own gap: the rebuilds, the lambda carried over and the kept states of every later iteration are in it); over 7 and 100
    iterations it stands within ten times the oracle builds' spread of the oracle's; no more iterations than asked for; a kind-3
    keyframe keeps its velocity and bias floats; with bInit every kind-0 keyframe holds the shared biases; a second call is bit-identical."""
    (p, pre), want = cases.scene(case), cases.case_oracle(case)
    kf, mp, b6, stats, chi2 = _call(opt, p, pre, case[2])
    at = cases.chi2_at(p, pre, dict(kfState=kf, mpPos=mp, bias6=b6))
    gap, spread = abs(at - chi2[1]) / max(1.0, chi2[1]), abs(chi2[1] - want["chi2"][1]) / max(1.0, want["chi2"][1])   # (relative to max(1, chi2), as every chi2 bound here)
    print(case[0], "stats4", stats.tolist(), "oracle", want["stats4"].tolist(), "chi2", chi2.tolist(), "oracle's", want["chi2"].tolist(),
          "chi2 at the state returned", at, "gap", gap, "to the oracle's", spread)
    assert abs(chi2[0] - want["chi2"][0]) <= 1e-9 * want["chi2"][0] and chi2[1] < chi2[0]
    assert stats[2:].tolist() == want["stats4"][2:].tolist() and 1 <= stats[0] <= case[2] and stats[0] <= stats[1] <= 10 * stats[0]
    assert gap <= 10 * cases.REEVAL_GAP
    if case in cases.FREE_PATH:
        assert spread <= 10 * cases.FREE_CHI2_SPREAD and stats[0] > 1
    kind, kf0 = p["kfKind"], np.ascontiguousarray(p["kfState"], np.float32)
    assert not np.isin(kind, (1, 2)).any() and np.isfinite(kf).all() and np.isfinite(mp).all()
    assert kf[kind == 3][:, 12:].tobytes() == kf0[kind == 3][:, 12:].tobytes()
    if p["init"]:
        assert (kf[kind == 0][:, 15:] == b6[None, :]).all()
    again = _call(opt, p, pre, case[2])
    for x, y in zip((kf, mp, b6, stats, chi2), again):
        assert x.tobytes() == y.tobytes()


def test_a_reused_handle_gives_the_bytes_of_a_fresh_one():
    """The handle's block is carved anew at every call: behind a larger problem, behind the visual global BA and behind MergeInertialBA a
    call finds other offsets and whatever they left, and must clear what its first kernels expect to be zero."""
    import global_ba_cases as gcases
    import merge_inertial_ba_cases as mcases
    from morb_slam_amd import Optimizer
    big, small, init = cases.GAUGED[0], cases.SMALL[4], cases.GAUGED_SMALL[3]
    g = gcases.scene(gcases.SMALL[1])
    mp_, mpre = mcases.problem("mix-3x1-s0")
    gba = lambda o: o.BundleAdjustment(g["kfPose"], g["kfFixed"], g["mpPos"], g["eKF"], g["eMP"], g["eObs"], g["eInvSigma2"], g["cam"])
    mib = lambda o: o.MergeInertialBA(mp_["kfState"], mp_["kfKind"], mp_["mpPos"], mp_["eKF"], mp_["eMP"], mp_["eObs"], mp_["eInvSigma2"],
                                      mp_["iKF1"], mp_["iKF2"], mpre, mp_["cam"], mp_["Tbc12"])
    fib = lambda c: (lambda o: _call(o, *cases.scene(c), c[2]))
    free = cases.FREE_PATH[2]            # (nothing fixed, bInit, 7 iterations: the call sites' configuration)
    calls = [fib(big), fib(small), gba, fib(free), fib(small), mib, fib(init), fib(free), fib(big), fib(small)]
    shared = Optimizer(0)
    try:
        for f in calls:
            fresh = Optimizer(0)
            try:
                a, b = f(shared), f(fresh)
            finally:
                fresh.close()
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
    finally:
        shared.close()


def test_stop_flag_set_at_entry(opt):
    case = cases.GAUGED[1]
    p, pre = cases.scene(case)
    kf, mp, b6, stats, chi2 = _call(opt, p, pre, case[2], stop_flag=np.array([1], np.uint8))
    assert stats.tolist() == [0, 0, 0, 0] and chi2.tolist() == [0, 0]
    assert kf.tobytes() == np.ascontiguousarray(p["kfState"], np.float32).tobytes() and mp.tobytes() == np.ascontiguousarray(p["mpPos"], np.float32).tobytes()
    assert b6.tobytes() == np.ascontiguousarray(p["bias6"], np.float32).tobytes()


@pytest.mark.parametrize("delay_us", [0, 300, 1500, 4000])
@pytest.mark.parametrize("free", [0, 1])
def test_stop_flag_raised_by_another_thread(opt, delay_us, free):
    """*pbStopFlag raised while the call runs: finite outputs, never more iterations than the undisturbed call.  The flag is one byte in
    the middle of a buffer whose other bytes are all set: were a neighbour read as the flag, the call would not run at all."""
    import time
    case = cases.FREE_PATH[1] if free else cases.GAUGED_LARGE      # (free: nothing fixed, 100 iterations asked for)
    (p, pre), want = cases.scene(case), cases.case_oracle(case)
    buf = np.full(64, 0xFF, np.uint8)
    buf[32] = 0
    flag = buf[32:33]

    def raiser():
        time.sleep(delay_us * 1e-6)   # (asleep, not spinning: a spinning thread holds the interpreter lock and the call would start late)
        flag[0] = 1
    th = threading.Thread(target=raiser)
    if delay_us:
        th.start()
    kf, mp, b6, stats, chi2 = _call(opt, p, pre, case[2], stop_flag=flag)
    if delay_us:
        th.join()
    print("delay", delay_us, "stats4", stats.tolist())
    if free:   # (the LM path may differ from the oracle's along the gauge: the bound is the call's own)
        assert stats[0] <= case[2] and stats[1] <= 10 * max(int(stats[0]), 1)
    else:
        assert stats[0] <= want["stats4"][0] and stats[1] <= want["stats4"][1]
    assert np.isfinite(kf).all() and np.isfinite(mp).all() and np.isfinite(chi2).all()
    if delay_us == 0:   # never raised: the neighbours' set bits were not taken for the flag
        assert stats[0] > 1 and (free or stats.tolist() == want["stats4"].tolist())


def _raw_args(p, pre):
    return dict(kf=np.ascontiguousarray(p["kfState"], np.float32).copy(), kind=np.ascontiguousarray(p["kfKind"], np.uint8).copy(),
                mp=np.ascontiguousarray(p["mpPos"], np.float32).copy(), eKF=p["eKF"].astype(np.int32).copy(), eMP=p["eMP"].astype(np.int32).copy(),
                obs=np.ascontiguousarray(p["eObs"], np.float32).copy(), inv=np.ascontiguousarray(p["eInvSigma2"], np.float32).copy(),
                i1=p["iKF1"].astype(np.int32).copy(), i2=p["iKF2"].astype(np.int32).copy(), pre=np.ascontiguousarray(pre, np.float32).copy(),
                tbc=np.ascontiguousarray(p["Tbc12"], np.float32).copy(), b6=np.ascontiguousarray(p["bias6"], np.float32).copy(),
                stats=np.full(4, -5, np.int32), chi2=np.full(2, -7.0, np.float64))


def _raw_call(opt, p, a, null=None, its=7, init=1, prior=(1e2, 1e6), **sizes):
    from morb_slam_amd.capi import lib, ptr
    g = lambda k: None if k == null else ptr(a[k])
    n = dict(nKF=len(a["kf"]), nMP=len(a["mp"]), nE=len(a["eKF"]), nI=len(a["i1"]))
    n.update(sizes)
    c = p["cam"]
    return lib().morb_full_inertial_ba(None if null == "handle" else opt._h, n["nKF"], g("kf"), g("kind"), n["nMP"], g("mp"), n["nE"], g("eKF"),
                                       g("eMP"), g("obs"), g("inv"), n["nI"], g("i1"), g("i2"), g("pre"), c["fx"], c["fy"], c["cx"], c["cy"],
                                       c["bf"], g("tbc"), its, init, prior[0], prior[1], g("b6"), None, g("stats"), g("chi2"))


def test_refused_calls(opt):
    """Each NULL, zero sizes, its out of range, indices out of range, a link ending on kind 2 or 3, a kind-0 keyframe without a link, NaN and
    Inf inputs: MORB_ERR_INVALID, every array untouched."""
    from morb_slam_amd.capi import HEADER
    INVALID = HEADER.constants["MORB_ERR_INVALID"]
    p, pre = cases.scene(cases.OBSERVERS)
    p = dict(p)
    kind = p["kfKind"].copy()
    kind[7] = 3                                    # (a kind-3 keyframe among the observers' scene: links 6-7 and 7-8 go)
    keep = (p["iKF1"] != 7) & (p["iKF2"] != 7)
    p.update(kfKind=kind, iKF1=p["iKF1"][keep], iKF2=p["iKF2"][keep])
    pre = pre[keep]

    def refused(rc, a, want):
        assert rc == INVALID, rc
        for k in want:
            assert a[k].tobytes() == want[k].tobytes(), k

    ref = _raw_args(p, pre)
    for null in ("handle", "kf", "kind", "mp", "eKF", "eMP", "obs", "inv", "i1", "i2", "pre", "tbc", "b6", "stats", "chi2"):
        a = _raw_args(p, pre)
        refused(_raw_call(opt, p, a, null=null), a, ref)
    for kw in (dict(nKF=0), dict(nMP=0), dict(nE=0), dict(nI=-1), dict(its=0), dict(its=101), dict(prior=(float("nan"), 1e6)), dict(prior=(1e2, float("inf")))):
        a = _raw_args(p, pre)
        refused(_raw_call(opt, p, a, **kw), a, ref)
    nKF, nMP = len(ref["kf"]), len(ref["mp"])
    edits = [("eKF", 0, nKF), ("eKF", 0, -1), ("eMP", 0, nMP), ("eMP", 0, -1), ("i1", 0, nKF), ("i2", 0, -1),
             ("i2", 0, int(np.flatnonzero(kind == 2)[0])), ("i2", 0, 7), ("i1", 1, int(p["iKF2"][1])),
             ("kind", 7, 0), ("kind", 3, 4),
             ("kf", 5, np.nan), ("mp", 4, np.inf), ("obs", 3, np.nan), ("inv", 2, np.inf), ("pre", 1, np.nan), ("tbc", 0, np.nan), ("b6", 5, np.inf)]
    for key, at, val in edits:
        a = _raw_args(p, pre)
        a[key].reshape(-1)[at] = val
        want = {k: v.copy() for k, v in a.items()}
        refused(_raw_call(opt, p, a), a, want)
    a = _raw_args(p, pre)   # and the untouched arguments do run; bias6 may be NULL without bInit
    assert _raw_call(opt, p, a) == 0 and a["stats"][0] >= 1 and a["chi2"][1] < a["chi2"][0]
    a = _raw_args(p, pre)
    assert _raw_call(opt, p, a, null="b6", init=0) == 0 and a["stats"][0] >= 1


def _star(n_kf, pairs):
    """n_kf keyframes of kind 3 and points seen as `pairs` lists them: finite numbers that are never looked at by a kernel."""
    kf = np.zeros((n_kf, 21), np.float32); kf[:, 0] = kf[:, 4] = kf[:, 8] = 1
    eKF = np.array([k for ks in pairs for k in ks], np.int32)
    eMP = np.array([m for m, ks in enumerate(pairs) for _ in ks], np.int32)
    nE = len(eKF)
    return dict(kfState=kf, kfKind=np.full(n_kf, 3, np.uint8), mpPos=np.ones((len(pairs), 3), np.float32), eKF=eKF, eMP=eMP,
                eObs=np.full((nE, 3), -1, np.float32), eInvSigma2=np.ones(nE, np.float32), iKF1=np.zeros(0, np.int32), iKF2=np.zeros(0, np.int32),
                Tbc12=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), bias6=np.zeros(6, np.float32),
                cam=dict(fx=400.0, fy=400.0, cx=300.0, cy=200.0, bf=40.0))


def test_capacity_refusals_come_before_any_launch(opt):
    """An envelope over the handle's byte cap (3400 pose-only keyframes that each share a point with keyframe 0: 6800 full block rows, 23.1 M
    blocks of 3 x 3 against 2^22 * 49 / 9) and more Schur contributions than an int indexes (one point seen by 32768 keyframes):
    MORB_ERR_CAPACITY, nothing written."""
    from morb_slam_amd.capi import HEADER
    CAPACITY = HEADER.constants["MORB_ERR_CAPACITY"]
    for p in (_star(3401, [[0, k] for k in range(1, 3401)]), _star(32768, [list(range(32768))])):
        a = _raw_args(p, np.zeros((0, 310), np.float32))
        want = {k: v.copy() for k, v in a.items()}
        rc = _raw_call(opt, p, a, init=0)
        assert rc == CAPACITY, rc
        for k in want:
            assert a[k].tobytes() == want[k].tobytes(), k
