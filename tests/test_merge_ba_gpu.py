"""The welding bundle adjustment of map merging on the GPU (morb_merge_bundle_adjustment*, Optimizer.MergeBundleAdjustment) against the CPU
oracle of tests/native/merge_ba_oracle.cc over the corpus of tests/merge_ba_cases.py; the stop flag; the refused calls."""
import threading

import numpy as np
import pytest

import merge_ba_cases as cases
import merge_ba_oracle as mo
from morb_slam_amd.synth import make_merge_ba_problem

pytestmark = pytest.mark.gpu
KEPT = [c for c in cases.CASES if c not in cases.LEFT_OUT]


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, stop_flag=None):
    return opt.MergeBundleAdjustment(p["kfPose"], p["kfFixed"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"],
                                     stop_flag=stop_flag, camL=p["camL"])


@pytest.mark.parametrize("case", KEPT, ids=cases.case_id)
def test_matches_the_oracle(opt, case):
    """Same LM path in both rounds (stats6), same level and erase flags, poses within 1e-4, points within 1e-4 relative to max(1, |X|), the
    fixed keyframes' bytes untouched, a second call bit-identical."""
    p, want = cases.scene(case), cases.case_oracle(case)
    kf, mp, erase, level, stats = _call(opt, p)
    print(cases.case_id(case), "edges", len(p["eKF"]), "stats6", stats.tolist(), "oracle", want["stats6"].tolist(),
          "pose", np.abs(kf - want["kfPose"]).max(), "points", (np.abs(mp - want["mpPos"]).max(1) / np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).max(),
          "level", int((level != want["level"]).sum()), "erase", int((erase != want["erase"]).sum()))
    assert stats.tolist() == want["stats6"].tolist()
    np.testing.assert_array_equal(level, want["level"])
    np.testing.assert_array_equal(erase, want["erase"])
    assert np.abs(kf - want["kfPose"]).max() <= 1e-4
    assert (np.abs(mp - want["mpPos"]).max(1) <= 1e-4 * np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).all()
    fixed = p["kfFixed"] != 0
    assert kf[fixed].tobytes() == np.ascontiguousarray(p["kfPose"], np.float32)[fixed].tobytes()
    again = _call(opt, p)
    for x, y in zip((kf, mp, erase, level, stats), again):
        assert x.tobytes() == y.tobytes()


def test_a_reused_workspace_gives_the_bytes_of_a_fresh_one():
    """The handle's `work` block is carved anew at every call (csrc/ba_host.h): behind a larger welding BA and behind a LocalBundleAdjustment a
    call finds other offsets and whatever they left; it must clear what it expects to find zero (the level mask, the round state)."""
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    from morb_slam_amd.synth import make_ba_problem
    big, small, b = cases.scene(cases.GRID[15]), cases.scene(cases.KEYFRAME_DROPS), make_ba_problem(8, 3, 500, seed=2)
    visual = lambda o: local_bundle_adjustment_oneshot(o, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    calls = [lambda o: _call(o, big), lambda o: _call(o, small), visual, lambda o: _call(o, small), visual]
    shared = Optimizer(0)
    try:
        for i, call in enumerate(calls):
            got = call(shared)
            fresh = Optimizer(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for x, y in zip(got, want):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), i
    finally:
        shared.close()


def test_stop_flag_set_at_entry(opt):
    p = cases.scene(cases.GRID[6])
    flag = np.zeros(4, np.uint8); flag[1:] = 255          # the neighbours of the bool are not read as part of it
    full = _call(opt, p, stop_flag=flag[:1])[4]
    assert full[5] == 2 and full[0] > 0
    flag[0] = 1
    kf, mp, erase, level, stats = _call(opt, p, stop_flag=flag[:1])
    assert stats.tolist() == [0] * 6 and not erase.any() and not level.any()
    assert kf.tobytes() == p["kfPose"].tobytes() and mp.tobytes() == p["mpPos"].tobytes()
    flag[0] = 0
    assert _call(opt, p, stop_flag=flag[:1])[4].tolist() == full.tolist()


def test_stop_flag_raised_by_another_thread(opt):
    """LoopClosing's flag arrives while the solve runs: the call returns with finite outputs and no more iterations than the undisturbed
    call; a call cut in round 1 has run one round, masked nothing and counted nothing for round 2."""
    p = make_merge_ba_problem(25, 25, 1500, seed=5)
    flag = np.zeros(4, np.uint8); flag[1:] = 255
    full = _call(opt, p, stop_flag=flag[:1])[4]
    assert full[5] == 2
    seen = set()
    for delay in (0.0, 2e-4, 1e-3, 3e-3):
        flag[0] = 0
        t = threading.Timer(delay, lambda: flag.__setitem__(0, 1))
        t.start()
        kf, mp, erase, level, stats = _call(opt, p, stop_flag=flag[:1])
        t.join()
        assert np.isfinite(kf).all() and np.isfinite(mp).all()
        assert stats[5] in (0, 1, 2) and stats[0] <= full[0] and stats[1] <= full[1] and stats[2] <= full[2] and stats[3] <= full[3]
        if stats[5] == 0:
            assert stats.tolist() == [0] * 6 and kf.tobytes() == p["kfPose"].tobytes()
        if stats[5] == 1:
            assert not level.any() and stats[2:5].tolist() == [0, 0, 0]
        seen.add(int(stats[5]))
    print("rounds run over the delays:", sorted(seen))


def test_invalid_arguments_are_refused(opt):
    from morb_slam_amd.capi import ERR_INVALID, lib, ptr
    L = lib()
    p = cases.scene(cases.GRID[0])
    a = [np.ascontiguousarray(p["kfPose"], np.float32).copy(), np.ascontiguousarray(p["kfFixed"], np.uint8), np.ascontiguousarray(p["mpPos"], np.float32).copy(),
         np.ascontiguousarray(p["eKF"], np.int32), np.ascontiguousarray(p["eMP"], np.int32), np.ascontiguousarray(p["eObs"], np.float32),
         np.ascontiguousarray(p["eInvSigma2"], np.float32)]
    c = p["cam"]
    nE = len(a[3])
    erase, level, stats = np.zeros(nE, np.uint8), np.zeros(nE, np.uint8), np.full(6, -7, np.int32)

    def call(kfPose=a[0], kfFixed=a[1], mpPos=a[2], eKF=a[3], eMP=a[4], eObs=a[5], inv=a[6], nKF=len(a[0]), nMP=len(a[2]), nE=nE, erase=erase, stats=stats, h=opt._h):
        q = lambda x: ptr(x) if x is not None else None
        return L.morb_merge_bundle_adjustment(h, nKF, q(kfPose), q(kfFixed), nMP, q(mpPos), nE, q(eKF), q(eMP), q(eObs), q(inv), c["fx"], c["fy"], c["cx"],
                                              c["cy"], c["bf"], None, q(erase), ptr(level), q(stats))

    for kw in (dict(h=None), dict(kfPose=None), dict(kfFixed=None), dict(mpPos=None), dict(eKF=None), dict(eMP=None), dict(eObs=None), dict(inv=None),
               dict(erase=None), dict(stats=None), dict(nE=0), dict(nKF=0), dict(nMP=0)):
        assert call(**kw) == ERR_INVALID, kw
    bad = a[3].copy(); bad[-1] = len(a[0])
    assert call(eKF=bad) == ERR_INVALID
    bad = a[4].copy(); bad[0] = -1
    assert call(eMP=bad) == ERR_INVALID
    c8 = np.zeros(8, np.float32)
    obs2 = np.ascontiguousarray(a[5][:, :2])
    f = lambda o2, cam: L.morb_merge_bundle_adjustment_fisheye(opt._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]), o2,
                                                              ptr(a[6]), cam, None, ptr(erase), ptr(level), ptr(stats))
    assert f(None, ptr(c8)) == ERR_INVALID and f(ptr(obs2), None) == ERR_INVALID
    assert stats.tolist() == [-7] * 6 and a[0].tobytes() == np.ascontiguousarray(p["kfPose"], np.float32).tobytes()
