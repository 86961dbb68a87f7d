"""Optimizer::BundleAdjustment(GlobalBAView&, int, bool, bool*) and the reference-typed WholeMapBundleAdjustment / GlobalBundleAdjustemnt
(include/morb/Optimizer.h with MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT defined), driven from C++ (tests/native/global_ba_adapter_check.cc): the view
call and the members on a mock map give the bytes of the C entry called from Python on the same problem, for both nLoopKF cases."""
import os
import subprocess

import numpy as np
import pytest

from morb_slam_amd.synth import make_global_ba_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("cam", ["mix", "kb8"])
def test_view_call_and_members_equal_the_c_entry(tmp_path, cam):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "global_ba_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_global_ba"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "global_ba_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    kb8 = cam == "kb8"
    p = make_global_ba_problem(8, 3, 120, 2, seed=70, kb8=kb8)
    nKF, nMP, nE = len(p["kfPose"]), len(p["mpPos"]), len(p["eKF"])
    assert len(np.unique(p["eMP"])) == nMP and len(np.unique(p["eKF"])) == nKF      # every vertex enters: the member's graph is this one
    c = p["cam"]
    camL = camR = np.zeros(8, np.float32)
    trl = np.array([0, 0, 0, 1, -0.1, 0, 0], np.float32)        # (the identity rotation survives the adapter's matrix -> quaternion step bit for bit)
    right = np.zeros(nE, np.uint8)
    obs3 = p["eObs"]
    if kb8:
        camL, camR, right = p["rig"]["camL"], p["rig"]["camR"], p["rig"]["eRight"]
        p["rig"] = dict(p["rig"], Trl=trl)
        obs3 = np.concatenate([p["eObs"], -np.ones((nE, 1), np.float32)], 1)
    else:
        camL = np.array([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], 0, 0, 0], np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nKF, nMP, nE, kb8], np.int32).tobytes() + np.ascontiguousarray(camL, np.float32).tobytes() + np.ascontiguousarray(camR, np.float32).tobytes() +
                trl.tobytes() + p["kfPose"].tobytes() + p["kfFixed"].tobytes() + p["mpPos"].tobytes() + p["eKF"].tobytes() + p["eMP"].tobytes() +
                np.ascontiguousarray(obs3, np.float32).tobytes() + np.ascontiguousarray(right, np.uint8).tobytes() + p["eInvSigma2"].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    opt = Optimizer(0)
    try:
        kf, mp, stats, chi2 = opt.BundleAdjustment(p["kfPose"], p["kfFixed"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"], rig=p["rig"])
    finally:
        opt.close()
    assert stats[0] > 1 and stats[2] == nKF - 1 and chi2[1] < chi2[0]
    # (1) the view-taking form
    assert take(np.float32, 7 * nKF).tobytes() == kf.tobytes() and take(np.float32, 3 * nMP).tobytes() == mp.tobytes()
    assert take(np.int32, 4).tolist() == stats.tolist() and take(np.float64, 2).tobytes() == chi2.tobytes()
    # (2) nLoopKF is the origin keyframe's: SetPose on every keyframe, SetWorldPos and UpdateNormalAndDepth on every point
    rec = take(np.dtype([("pose", np.float32, 7), ("n", np.int32)]), nKF)
    assert rec["pose"].tobytes() == kf.tobytes() and (rec["n"] == 1).all()
    rec = take(np.dtype([("pos", np.float32, 3), ("n", np.int32)]), nMP)
    assert rec["pos"].tobytes() == mp.tobytes() and (rec["n"] == 1).all()
    # (3) another nLoopKF (5): mTcwGBA / mPosGBA and the mark, no SetPose, no UpdateNormalAndDepth
    rec = take(np.dtype([("pose", np.float32, 7), ("n", np.int32)]), nKF)
    assert rec["pose"].tobytes() == kf.tobytes() and (rec["n"] == 5).all()
    rec = take(np.dtype([("pos", np.float32, 3), ("n", np.int32)]), nMP)
    assert rec["pos"].tobytes() == mp.tobytes() and (rec["n"] == 5).all()
    assert off == len(raw)
