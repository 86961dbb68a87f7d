"""MergeInertialBA on the GPU (morb_merge_inertial_ba*, Optimizer.MergeInertialBA) against the CPU oracle of
tests/native/merge_inertial_ba_oracle.cc over the corpus of tests/merge_inertial_ba_cases.py; workspace reuse; the stop flag; the refused
calls; and LocalInertialBA, which shares the kernels, against the bytes recorded before they changed."""
import hashlib
import os
import threading

import numpy as np
import pytest

import merge_inertial_ba_cases as cases
from morb_slam_amd.synth import imu_calib_diagonals, make_inertial_ba_problem

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_inertial_ba_parent.npz")


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, pre, stop_flag=None):
    return opt.MergeInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"], pre,
                               p["cam"], p["Tbc12"], stop_flag=stop_flag, rig=p["rig28"])


@pytest.mark.parametrize("name", cases.KEPT)
def test_matches_the_oracle(opt, name):
    """Same LM path (stats3), same erase flags, 15-dof states and 6-dof poses within 1e-4, points within 1e-4 relative to max(1, |X|); kinds
    1 / 2 keep every byte and kind 3 its velocity / bias floats; a second call is bit-identical."""
    (p, pre), want = cases.problem(name), cases.oracle(name)
    kf, mp, erase, stats = _call(opt, p, pre)
    kind, kf0 = p["kfKind"], np.ascontiguousarray(p["kfState"], np.float32)
    d15 = np.abs(kf[kind == 0] - want["kfState"][kind == 0]).max()
    d6 = np.abs(kf[kind == 3][:, :12] - want["kfState"][kind == 3][:, :12]).max() if (kind == 3).any() else 0.0
    dp = (np.abs(mp - want["mpPos"]).max(1) / np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).max()
    print(name, "edges", len(erase), "stats3", stats.tolist(), "oracle", want["stats3"].tolist(), "15-dof", d15, "6-dof", d6, "points", dp,
          "erase", int((erase != want["erase"]).sum()))
    assert stats.tolist() == want["stats3"].tolist()
    np.testing.assert_array_equal(erase, want["erase"])
    assert d15 <= 1e-4 and d6 <= 1e-4 and dp <= 1e-4
    fixed = (kind == 1) | (kind == 2)
    assert kf[fixed].tobytes() == kf0[fixed].tobytes()
    assert kf[kind == 3][:, 12:].tobytes() == kf0[kind == 3][:, 12:].tobytes()
    if (kind == 3).any():
        moved = not np.array_equal(want["kfState"][kind == 3][:, :12], kf0[kind == 3][:, :12])   # (they do, but where the only trial is undone)
        assert moved == (name != "ends-rejected") and moved == (not np.array_equal(kf[kind == 3][:, :12], kf0[kind == 3][:, :12]))
    again = _call(opt, p, pre)
    for x, y in zip((kf, mp, erase, stats), again):
        assert x.tobytes() == y.tobytes()


def _local_problem(n_opt, n_points, seed, rig=False):
    import oracle_lib as orc
    nga, walk = imu_calib_diagonals()
    p = make_inertial_ba_problem(n_opt=n_opt, n_points=n_points, seed=seed, rig=rig)
    pre = np.stack([orc.imu_preintegrate(p["bias"], nga, walk, p["acc"][a:b], p["gyro"][a:b], p["dt"][a:b])
                    for a, b in zip(p["imuStart"][:-1], p["imuStart"][1:])])
    return p, pre


def _local(opt, p, pre):
    rig = p["rig28"] is not None
    return opt.LocalInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["mpClose"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"],
                               p["iKF2"], pre, p["iRobust"], p["iInfoScale"], None if rig else p["cam"], p["Tbc12"],
                               rig=p["rig28"] if rig else None, eRight=p["eRight"] if rig else None)


def test_a_reused_workspace_gives_the_bytes_of_a_fresh_one():
    """The handle's `work` block is carved anew at every call: behind a larger MergeInertialBA, behind LocalInertialBA and behind the visual
    welding BA a call finds other offsets and whatever they left, and must clear what its first kernels expect to be zero."""
    from morb_slam_amd import Optimizer
    from morb_slam_amd.synth import make_merge_ba_problem
    big, small = cases.problem("mix-13x30-s0"), cases.problem("mix-3x1-s0")
    lp = _local_problem(4, 400, 0)
    w = make_merge_ba_problem(6, 6, 300, seed=1)
    weld = lambda o: o.MergeBundleAdjustment(w["kfPose"], w["kfFixed"], w["mpPos"], w["eKF"], w["eMP"], w["eObs"], w["eInvSigma2"], w["cam"])
    calls = [lambda o: _call(o, *big), lambda o: _call(o, *small), lambda o: _local(o, *lp), lambda o: _call(o, *small), weld,
             lambda o: _call(o, *small), lambda o: _local(o, *lp)]
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
    p, pre = cases.problem("mix-3x1-s0")
    flag = np.array([1], np.uint8)
    kf, mp, erase, stats = _call(opt, p, pre, stop_flag=flag)
    assert stats.tolist() == [0, 0, 0] and not erase.any()
    assert kf.tobytes() == np.ascontiguousarray(p["kfState"], np.float32).tobytes() and mp.tobytes() == np.ascontiguousarray(p["mpPos"], np.float32).tobytes()


@pytest.mark.parametrize("delay_us", [0, 300, 800, 1500, 2500])
def test_stop_flag_raised_by_another_thread(opt, delay_us):
    """*pbStopFlag raised while the call runs: finite outputs, never more iterations than the undisturbed call.  The flag is one byte in
    the middle of a buffer whose other bytes are all set: were a neighbour read as the flag, the call would not run at all."""
    import time
    p, pre = cases.problem("mix-13x30-s0")
    want = cases.oracle("mix-13x30-s0")
    buf = np.full(64, 0xFF, np.uint8)
    buf[32] = 0
    flag = buf[32:33]

    def raiser():
        time.sleep(delay_us * 1e-6)   # (asleep, not spinning: a spinning thread holds the interpreter lock and the call would start late)
        flag[0] = 1
    th = threading.Thread(target=raiser)
    if delay_us:
        th.start()
    kf, mp, erase, stats = _call(opt, p, pre, stop_flag=flag)
    if delay_us:
        th.join()
    print("delay", delay_us, "stats3", stats.tolist())
    assert stats[2] == 1 or delay_us
    assert stats[0] <= want["stats3"][0] and stats[1] <= want["stats3"][1]
    assert np.isfinite(kf).all() and np.isfinite(mp).all()
    if delay_us == 0:   # never raised: the neighbours' set bits were not taken for the flag
        assert stats.tolist() == want["stats3"].tolist()


def _raw_args(p, pre):
    a = dict(kf=np.ascontiguousarray(p["kfState"], np.float32).copy(), kind=np.ascontiguousarray(p["kfKind"], np.uint8).copy(),
             mp=np.ascontiguousarray(p["mpPos"], np.float32).copy(), eKF=p["eKF"].astype(np.int32).copy(), eMP=p["eMP"].astype(np.int32).copy(),
             obs=np.ascontiguousarray(p["eObs"], np.float32).copy(), inv=np.ascontiguousarray(p["eInvSigma2"], np.float32).copy(),
             i1=p["iKF1"].astype(np.int32).copy(), i2=p["iKF2"].astype(np.int32).copy(), pre=np.ascontiguousarray(pre, np.float32).copy(),
             tbc=np.ascontiguousarray(p["Tbc12"], np.float32).copy(), erase=np.full(len(p["eKF"]), 7, np.uint8), stats=np.full(3, -5, np.int32))
    return a


def _raw_call(opt, p, a, null=None, **sizes):
    from morb_slam_amd.capi import lib, ptr
    g = lambda k: None if k == null else ptr(a[k])
    n = dict(nKF=len(a["kf"]), nMP=len(a["mp"]), nE=len(a["eKF"]), nI=len(a["i1"]))
    n.update(sizes)
    c = p["cam"]
    return lib().morb_merge_inertial_ba(None if null == "handle" else opt._h, n["nKF"], g("kf"), g("kind"), n["nMP"], g("mp"), n["nE"], g("eKF"),
                                        g("eMP"), g("obs"), g("inv"), n["nI"], g("i1"), g("i2"), g("pre"), c["fx"], c["fy"], c["cx"], c["cy"],
                                        c["bf"], g("tbc"), None, g("erase"), g("stats"))


def test_refused_calls(opt):
    """Each NULL, zero sizes, indices out of range, a link ending on kind 2 or 3: MORB_ERR_INVALID, stats3 and every array untouched."""
    from morb_slam_amd.capi import HEADER
    INVALID = HEADER.constants["MORB_ERR_INVALID"]
    p, pre = cases.problem("observers")
    ref = _raw_args(p, pre)

    def refused(rc, a):
        assert rc == INVALID, rc
        for k in ref:
            assert a[k].tobytes() == ref[k].tobytes(), k

    for null in ("handle", "kf", "kind", "mp", "eKF", "eMP", "obs", "inv", "i1", "i2", "pre", "tbc", "erase", "stats"):
        a = _raw_args(p, pre)
        refused(_raw_call(opt, p, a, null=null), a)
    for sizes in (dict(nKF=0), dict(nMP=0), dict(nE=0), dict(nI=-1)):
        a = _raw_args(p, pre)
        refused(_raw_call(opt, p, a, **sizes), a)
    nKF, nMP = len(ref["kf"]), len(ref["mp"])
    for key, val in (("eKF", nKF), ("eKF", -1), ("eMP", nMP), ("eMP", -1), ("i1", nKF), ("i2", -1)):
        a = _raw_args(p, pre)
        a[key][0] = val
        want = {k: v.copy() for k, v in a.items()}
        rc = _raw_call(opt, p, a)
        assert rc == INVALID and all(a[k].tobytes() == want[k].tobytes() for k in a), (key, val, rc)
    kind = p["kfKind"]
    for bad_kind in (2, 3):
        a = _raw_args(p, pre)
        a["i2"][0] = int(np.where(kind == bad_kind)[0][0])
        want = {k: v.copy() for k, v in a.items()}
        rc = _raw_call(opt, p, a)
        assert rc == INVALID and all(a[k].tobytes() == want[k].tobytes() for k in a), (bad_kind, rc)
    a = _raw_args(p, pre)   # and the untouched arguments do run
    assert _raw_call(opt, p, a) == 0 and a["stats"][2] == 1


def test_local_inertial_ba_gives_the_bytes_recorded_before_the_kernels_were_shared(opt):
    """morb_local_inertial_ba and _fisheye on make_inertial_ba_problem(n_opt=4, n_points=400, seed=0) and (n_opt=10, seed=1): states, erase
    flags, stats and points (by SHA-256) are those the library gave before inertial_ba.hip learnt MergeInertialBA's graph
    (tests/golden/local_inertial_ba_parent.npz), byte for byte."""
    g = np.load(GOLDEN)
    for name, (n_opt, n_points, seed) in (("a", (4, 400, 0)), ("b", (10, 1500, 1))):
        for rig in (False, True):
            p, pre = _local_problem(n_opt, n_points, seed, rig=rig)
            kf, mp, er, st = _local(opt, p, pre)
            key = name + ("_rig" if rig else "")
            assert st.tolist() == g[key + "_stats"].tolist(), key
            assert kf.tobytes() == g[key + "_kf"].tobytes(), (key, np.abs(kf - g[key + "_kf"]).max())
            assert np.packbits(er).tobytes() == g[key + "_erase"].tobytes(), key
            assert mp[:16].tobytes() == g[key + "_mp_head"].tobytes(), key
            assert hashlib.sha256(mp.tobytes()).digest() == g[key + "_mp_sha256"].tobytes(), key
