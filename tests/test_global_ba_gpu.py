"""The whole-map bundle adjustment of loop closing on the GPU (morb_bundle_adjustment*, Optimizer.BundleAdjustment) against the CPU oracle of
tests/native/global_ba_oracle.cc over the corpus of tests/global_ba_cases.py; the reused handle; the stop flag; the refused calls."""
import threading

import numpy as np
import pytest

import global_ba_cases as cases

KEPT = [c for c in cases.CASES if c not in cases.LEFT_OUT]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer()
    yield o
    o.close()


def _call(opt, p, n_iterations=10, robust=False, stop_flag=None):
    return opt.BundleAdjustment(p["kfPose"], p["kfFixed"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"],
                                n_iterations=n_iterations, robust=robust, stop_flag=stop_flag, rig=p["rig"])


@pytest.mark.parametrize("case", KEPT, ids=cases.case_id)
def test_matches_the_oracle(opt, case):
    """Same LM path (outer iterations, trials), same system (keyframes, envelope blocks), poses within 1e-4, points within 1e-4 relative to
    max(1, |X|), chi2 within cases.CHI2_MARGIN, the bytes of fixed keyframes, keyframes without an edge and points without an edge kept, a second
    call bit-identical."""
    p, want = cases.scene(case), cases.case_oracle(case)
    kf, mp, stats, chi2 = _call(opt, p, case[6], bool(case[5]))
    rel = np.abs(chi2 - want["chi2"]) / np.maximum(want["chi2"], cases.CHI2_FLOOR)
    print(cases.case_id(case), "edges", len(p["eKF"]), "stats4", stats.tolist(), "oracle", want["stats4"].tolist(),
          "pose", np.abs(kf - want["kfPose"]).max(), "points", (np.abs(mp - want["mpPos"]).max(1) / np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).max(),
          "chi2", chi2.tolist(), "oracle", want["chi2"].tolist(), "relative", rel.tolist())
    assert stats.tolist() == want["stats4"].tolist()
    assert np.abs(kf - want["kfPose"]).max() <= 1e-4
    assert (np.abs(mp - want["mpPos"]).max(1) <= 1e-4 * np.maximum(1.0, np.linalg.norm(want["mpPos"], axis=1))).all()
    assert (np.abs(chi2 - want["chi2"]) <= cases.CHI2_MARGIN * want["chi2"] + cases.CHI2_FLOOR).all()
    used = np.zeros(len(kf), bool); used[p["eKF"]] = True
    keep = (p["kfFixed"] != 0) | ~used
    assert keep.any() and kf[keep].tobytes() == np.ascontiguousarray(p["kfPose"], np.float32)[keep].tobytes()
    idle = np.setdiff1d(np.arange(len(mp)), p["eMP"])
    assert mp[idle].tobytes() == np.ascontiguousarray(p["mpPos"], np.float32)[idle].tobytes()
    again = _call(opt, p, case[6], bool(case[5]))
    for x, y in zip((kf, mp, stats, chi2), again):
        assert x.tobytes() == y.tobytes()


def test_a_reused_handle_gives_the_bytes_of_a_fresh_one():
    """The handle's blocks are carved anew at every call (csrc/ba_host.h): behind a larger call and behind a LocalBundleAdjustment, which
    shares the pinned staging buffer and the mapped LM words, a call finds other offsets and whatever they left."""
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    from morb_slam_amd.synth import make_ba_problem
    big, small, rig, b = cases.scene(cases.SHAPES[2]), cases.scene(cases.IDLE), cases.scene(cases.SMALL[17]), make_ba_problem(8, 3, 500, seed=2)
    visual = lambda o: local_bundle_adjustment_oneshot(o, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    calls = [lambda o: _call(o, big), lambda o: _call(o, small), visual, lambda o: _call(o, small, robust=True), lambda o: _call(o, rig), visual]
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
    p = cases.scene(cases.SHAPES[0])
    flag = np.zeros(4, np.uint8); flag[1:] = 255          # the neighbours of the bool are not read as part of it
    full = _call(opt, p, stop_flag=flag[:1])
    assert full[2][0] > 0
    flag[0] = 1
    kf, mp, stats, chi2 = _call(opt, p, stop_flag=flag[:1])
    assert stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
    assert kf.tobytes() == p["kfPose"].tobytes() and mp.tobytes() == p["mpPos"].tobytes()
    flag[0] = 0
    for x, y in zip(full, _call(opt, p, stop_flag=flag[:1])):
        assert x.tobytes() == y.tobytes()


def test_stop_flag_raised_by_another_thread(opt):
    """LoopClosing's flag arrives while the solve runs: the call returns with finite outputs and no more iterations or trials than the
    undisturbed call."""
    p = cases.scene(cases.LARGE[0])
    flag = np.zeros(4, np.uint8); flag[1:] = 255
    full = _call(opt, p, stop_flag=flag[:1])[2]
    seen = set()
    for delay in (0.0, 3e-4, 1e-3, 3e-3):
        flag[0] = 0
        t = threading.Timer(delay, lambda: flag.__setitem__(0, 1))
        t.start()
        kf, mp, stats, chi2 = _call(opt, p, stop_flag=flag[:1])
        t.join()
        assert np.isfinite(kf).all() and np.isfinite(mp).all() and np.isfinite(chi2).all()
        assert stats[0] <= full[0] and stats[1] <= full[1]
        if stats[2] == 0:          # the flag was up at entry
            assert stats.tolist() == [0] * 4 and kf.tobytes() == p["kfPose"].tobytes()
        else:
            assert stats[2:].tolist() == full[2:].tolist() and chi2[1] <= chi2[0]
        seen.add(int(stats[0]))
    print("outer iterations over the delays:", sorted(seen), "undisturbed:", int(full[0]))


def _arrays(p):
    return dict(kfPose=np.ascontiguousarray(p["kfPose"], np.float32).copy(), kfFixed=np.ascontiguousarray(p["kfFixed"], np.uint8),
                mpPos=np.ascontiguousarray(p["mpPos"], np.float32).copy(), eKF=np.ascontiguousarray(p["eKF"], np.int32),
                eMP=np.ascontiguousarray(p["eMP"], np.int32), eObs=np.ascontiguousarray(p["eObs"], np.float32),
                inv=np.ascontiguousarray(p["eInvSigma2"], np.float32))


def _raw(opt, a, cam, stats, chi2, n_iterations=10, h=True, **kw):
    from morb_slam_amd.capi import lib, ptr
    b = dict(a); b.update(kw)
    q = lambda x: ptr(x) if x is not None else None
    return lib().morb_bundle_adjustment(opt._h if h else None, b.get("nKF", len(a["kfPose"])), q(b["kfPose"]), q(b["kfFixed"]), b.get("nMP", len(a["mpPos"])),
                                        q(b["mpPos"]), b.get("nE", len(a["eKF"])), q(b["eKF"]), q(b["eMP"]), q(b["eObs"]), q(b["inv"]), cam["fx"], cam["fy"],
                                        cam["cx"], cam["cy"], cam["bf"], n_iterations, 0, None, q(stats), q(chi2))


def test_invalid_arguments_are_refused(opt):
    from morb_slam_amd.capi import ERR_INVALID, lib, ptr
    p = cases.scene(cases.SMALL[2])
    a, c = _arrays(p), p["cam"]
    stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)
    call = lambda **kw: _raw(opt, a, c, kw.pop("stats", stats), kw.pop("chi2", chi2), **kw)
    for kw in (dict(h=False), dict(kfPose=None), dict(kfFixed=None), dict(mpPos=None), dict(eKF=None), dict(eMP=None), dict(eObs=None), dict(inv=None),
               dict(stats=None), dict(chi2=None), dict(nE=0), dict(nKF=0), dict(nMP=0), dict(n_iterations=0), dict(n_iterations=101)):
        assert call(**kw) == ERR_INVALID, kw
    bad = a["eKF"].copy(); bad[-1] = len(a["kfPose"])
    assert call(eKF=bad) == ERR_INVALID
    bad = a["eMP"].copy(); bad[0] = -1
    assert call(eMP=bad) == ERR_INVALID
    for key, at, v in (("kfPose", (1, 5), np.nan), ("kfPose", (0, 0), np.inf), ("mpPos", (3, 2), np.nan), ("eObs", (7, 1), -np.inf), ("eObs", (2, 2), np.nan),
                       ("inv", (4,), np.inf)):
        bad = a[key].copy(); bad[at] = v
        assert call(**{key: bad}) == ERR_INVALID, (key, v)
    r = cases.scene(cases.SMALL[17])
    ra = _arrays(r)
    f = lambda **kw: lib().morb_bundle_adjustment_fisheye(opt._h, len(ra["kfPose"]), ptr(ra["kfPose"]), ptr(ra["kfFixed"]), len(ra["mpPos"]), ptr(ra["mpPos"]),
                                                          len(ra["eKF"]), ptr(ra["eKF"]), ptr(ra["eMP"]), *[None if k in kw else ptr(np.ascontiguousarray(v)) for k, v in
                                                          (("obs", ra["eObs"]), ("right", r["rig"]["eRight"]), ("inv", ra["inv"]), ("camL", r["rig"]["camL"]),
                                                           ("camR", r["rig"]["camR"]), ("Trl", r["rig"]["Trl"]))], 10, 0, None, ptr(stats), ptr(chi2))
    for k in ("obs", "right", "inv", "camL", "camR", "Trl"):
        assert f(**{k: None}) == ERR_INVALID, k
    assert stats.tolist() == [-7] * 4 and chi2.tolist() == [-7.0] * 2
    assert a["kfPose"].tobytes() == np.ascontiguousarray(p["kfPose"], np.float32).tobytes() and a["mpPos"].tobytes() == p["mpPos"].tobytes()
    assert ra["kfPose"].tobytes() == np.ascontiguousarray(r["kfPose"], np.float32).tobytes()


def test_no_free_keyframe_with_an_edge_is_ok_and_writes_nothing(opt):
    from morb_slam_amd.capi import MORB_OK as OK
    p = cases.scene(cases.SMALL[2])
    a, c = _arrays(p), p["cam"]
    stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)
    assert _raw(opt, a, c, stats, chi2, kfFixed=np.ones(len(a["kfPose"]), np.uint8)) == OK
    assert stats.tolist() == [0] * 4 and chi2.tolist() == [0.0, 0.0]
    assert a["kfPose"].tobytes() == np.ascontiguousarray(p["kfPose"], np.float32).tobytes() and a["mpPos"].tobytes() == p["mpPos"].tobytes()


def test_capacity_is_refused_before_any_launch(opt):
    """An envelope of more blocks than the handle may grow to (3400 free keyframes that each share a point with the first: 3400 * 3401 / 2
    blocks against 2^22 * 49 / 36), and a Schur complement of more pair contributions than an int indexes (478 points each seen by 3000
    free keyframes: 478 * 3000 * 3001 / 2 > 2^31): MORB_ERR_CAPACITY, nothing written."""
    from morb_slam_amd.capi import ERR_CAPACITY
    cam = cases.scene(cases.SMALL[0])["cam"]
    for n_free, n_pts, wide in ((3400, 3400, False), (3000, 478, True)):
        nKF = n_free + 1
        if wide:
            eKF = np.tile(np.arange(1, nKF, dtype=np.int32), n_pts); eMP = np.repeat(np.arange(n_pts, dtype=np.int32), n_free)
        else:
            eKF = np.stack([np.ones(n_pts, np.int32), np.arange(1, nKF, dtype=np.int32)], 1).ravel(); eMP = np.repeat(np.arange(n_pts, dtype=np.int32), 2)
        kf = np.zeros((nKF, 7), np.float32); kf[:, 3] = 1
        fixed = np.zeros(nKF, np.uint8); fixed[0] = 1
        a = dict(kfPose=kf, kfFixed=fixed, mpPos=np.ones((n_pts, 3), np.float32) * 5, eKF=eKF, eMP=eMP,
                 eObs=np.tile(np.array([300, 200, -1], np.float32), (len(eKF), 1)), inv=np.ones(len(eKF), np.float32))
        keep = a["kfPose"].copy()
        stats, chi2 = np.full(4, -7, np.int32), np.full(2, -7.0)
        assert _raw(opt, a, cam, stats, chi2) == ERR_CAPACITY, n_free
        assert stats.tolist() == [-7] * 4 and chi2.tolist() == [-7.0] * 2 and a["kfPose"].tobytes() == keep.tobytes() and (a["mpPos"] == 5).all()
