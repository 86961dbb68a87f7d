"""Optimizer::FullInertialBA(FullInertialBAView&, ...) and the reference-typed FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit,
priorG, priorA) (include/morb/Optimizer.h), driven from C++ (tests/native/full_inertial_ba_adapter_check.cc): the view call and the member on a
mock map give the bytes of the C entry called from Python on the same problem — states, velocities, biases, points, stats and chi2, the poses
through Tcw = (Rcb Rwb^T, tcb - Rcb Rwb^T twb) — for both write-backs, with the shared bias of bInit on every keyframe with an IMU."""
import os
import subprocess

import numpy as np
import pytest

import full_inertial_ba_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("case", cases.CUT, ids=cases.case_id)
def test_view_call_and_member_equal_the_c_entry(tmp_path, case):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "full_inertial_ba_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_full_inertial_ba"), "-I" + os.path.join(NATIVE, "mock_ref"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "full_inertial_ba_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p, pre = cases.scene(case)
    its, init = case[2], p["init"]
    nKF, nMP, nE, nI = len(p["kfState"]), len(p["mpPos"]), len(p["eKF"]), len(p["iKF1"])
    kind = p["kfKind"]
    assert set(kind.tolist()) == {0, 3} and (np.diff(p["iKF2"]) > 0).all()   # the member's graph is this one
    seen = np.zeros(nMP, bool); seen[p["eMP"]] = True
    rig = p["rig28"] is not None
    c = p["cam"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    bias_in = np.ascontiguousarray(p["kfState"], np.float32)[-1, 15:].copy()          # pIncKF: the last keyframe's bias
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nKF, nMP, nE, nI, rig, its, init], np.int32).tobytes() + f32([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"]]) +
                f32(p["rig28"] if rig else np.zeros(28)) + f32(p["Tbc12"]) + f32([p["priorG"], p["priorA"]]) + f32(bias_in) + f32(p["kfState"]) +
                kind.astype(np.uint8).tobytes() + f32(p["mpPos"]) + p["eKF"].astype(np.int32).tobytes() + p["eMP"].astype(np.int32).tobytes() +
                f32(p["eObs"]) + p["eRight"].astype(np.uint8).tobytes() + f32(p["eInvSigma2"]) + p["iKF1"].astype(np.int32).tobytes() +
                p["iKF2"].astype(np.int32).tobytes() + f32(pre))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "full inertial ba adapter ok" in r.stdout, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    opt = Optimizer(0)
    try:
        kf, mp, b6, stats, chi2 = opt.FullInertialBA(p["kfState"], kind, p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"],
                                                     pre, p["cam"], p["Tbc12"], its=its, init=init, prior_g=p["priorG"], prior_a=p["priorA"],
                                                     bias6=bias_in, rig=p["rig28"], eRight=p["eRight"] if rig else None)
    finally:
        opt.close()
    assert stats[0] >= 1 and chi2[1] < chi2[0] and not np.array_equal(kf, np.ascontiguousarray(p["kfState"], np.float32))
    # (1) the view-taking form
    assert take(np.float32, 21 * nKF).tobytes() == kf.tobytes() and take(np.float32, 3 * nMP).tobytes() == mp.tobytes()
    assert take(np.float32, 6).tobytes() == b6.tobytes() and take(np.int32, 4).tolist() == stats.tolist() and take(np.float64, 2).tobytes() == chi2.tobytes()
    # (2) nLoopId == 0, no stop flag: the keyframes' and points' own members; (3) a loop id (5) and a stop flag: the GBA members
    Tbc = np.ascontiguousarray(p["Tbc12"], np.float32).astype(np.float64)
    rec = np.dtype([("n", np.int32, 4), ("R", np.float32, 9), ("t", np.float32, 3), ("v", np.float32, 3), ("b", np.float32, 6)])
    prec = np.dtype([("n", np.int32, 2), ("X", np.float32, 3)])
    imu = kind == 0
    for run in (0, 1):
        K = take(np.uint8, rec.itemsize * nKF).view(rec)
        M = take(np.uint8, prec.itemsize * nMP).view(prec)
        nbias, changes = take(np.int32, nI), take(np.int32, 1)[0]
        assert changes == 1 and nbias.tolist() == [1] * nI
        for k in range(nKF):
            want = [1, int(imu[k]), int(imu[k]), 0] if run == 0 else [0, 0, 0, 5]
            assert K["n"][k].tolist() == want, (run, k, K["n"][k])
            st = kf[k].astype(np.float64)
            Rcw, tcw = np.zeros(9), np.zeros(3)          # the member's own sums, term by term
            for r_ in range(3):
                for c_ in range(3):
                    a = 0.0
                    for i in range(3):
                        a += Tbc[3 * i + r_] * st[3 * c_ + i]
                    Rcw[3 * r_ + c_] = a
            for r_ in range(3):
                a = 0.0
                for i in range(3):
                    a -= Tbc[3 * i + r_] * Tbc[9 + i]
                for c_ in range(3):
                    a -= Rcw[3 * r_ + c_] * st[9 + c_]
                tcw[r_] = a
            assert K["R"][k].tobytes() == Rcw.astype(np.float32).tobytes() and K["t"][k].tobytes() == tcw.astype(np.float32).tobytes(), (run, k)
            if imu[k]:   # velocity, and the bias: the keyframe's own, or with bInit the shared one
                assert K["v"][k].tobytes() == kf[k][12:15].tobytes() and K["b"][k].tobytes() == (b6 if init else kf[k][15:]).tobytes(), (run, k)
            elif run == 0:
                assert np.concatenate([K["v"][k], K["b"][k]]).tobytes() == np.ascontiguousarray(p["kfState"], np.float32)[k][12:].tobytes()
        assert M["X"][seen].tobytes() == mp[seen].tobytes()
        assert M["n"].tolist() == [([1, 0] if run == 0 else [0, 5]) if s else [0, 0] for s in seen]      # (a point nobody sees is not in the graph)
    assert off == len(raw)
