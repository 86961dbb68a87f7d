"""Optimizer::LocalBundleAdjustment(MergeBAView&, bool*) and the reference-typed LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF,
pbStopFlag) (include/morb/Optimizer.h), driven from C++ (tests/native/merge_ba_adapter_check.cc): the view call gives the bytes of the C
entry called from Python on the same problem, and the mock-map member — which walks the fixed window first and takes the points in the order
its keyframes hold them — the bytes of the C entry on the problem flattened that way."""
import os
import subprocess

import numpy as np
import pytest

from morb_slam_amd.synth import make_merge_ba_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _as_the_member_flattens(p):
    """The problem in the member's order: fixed keyframes, then free ones; points by first appearance over the keyframes in that order (each
    keyframe's points ascending); edges by point, a point's observations by keyframe.  Returns (problem, keyframe order, point order, edge order)."""
    nKF = len(p["kfPose"])
    kf_order = [k for k in range(nKF) if p["kfFixed"][k]] + [k for k in range(nKF) if not p["kfFixed"][k]]
    mp_order, seen = [], set()
    for k in kf_order:
        for j in sorted(set(p["eMP"][p["eKF"] == k].tolist())):
            if j not in seen:
                seen.add(j); mp_order.append(j)
    kf_new = {k: i for i, k in enumerate(kf_order)}
    mp_new = {j: i for i, j in enumerate(mp_order)}
    e_order = sorted(range(len(p["eKF"])), key=lambda e: (mp_new[int(p["eMP"][e])], int(p["eKF"][e]), e))
    q = dict(p)
    q.update(kfPose=p["kfPose"][kf_order], kfFixed=p["kfFixed"][kf_order], mpPos=p["mpPos"][mp_order],
             eKF=np.array([kf_new[int(p["eKF"][e])] for e in e_order], np.int32), eMP=np.array([mp_new[int(p["eMP"][e])] for e in e_order], np.int32),
             eObs=p["eObs"][e_order], eInvSigma2=p["eInvSigma2"][e_order])
    return q, kf_order, mp_order, e_order


@pytest.mark.parametrize("cam", ["mix", "kb8"])
def test_view_call_and_member_equal_the_c_entry(tmp_path, cam):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "merge_ba_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_merge_ba"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "merge_ba_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p = make_merge_ba_problem(5, 3, 200, seed=70, kb8=cam == "kb8")
    nKF, nMP, nE = len(p["kfPose"]), len(p["mpPos"]), len(p["eKF"])
    obs3 = p["eObs"] if cam != "kb8" else np.concatenate([p["eObs"], -np.ones((nE, 1), np.float32)], 1)
    c = p["cam"]
    cam8 = p["camL"] if cam == "kb8" else np.array([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], 0, 0, 0], np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nKF, nMP, nE, cam == "kb8"], np.int32).tobytes() + np.ascontiguousarray(cam8, np.float32).tobytes() + p["kfPose"].tobytes() +
                p["kfFixed"].tobytes() + p["mpPos"].tobytes() + p["eKF"].tobytes() + p["eMP"].tobytes() + np.ascontiguousarray(obs3, np.float32).tobytes() +
                p["eInvSigma2"].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    call = lambda o, q: o.MergeBundleAdjustment(q["kfPose"], q["kfFixed"], q["mpPos"], q["eKF"], q["eMP"], q["eObs"], q["eInvSigma2"], q["cam"], camL=q["camL"])
    opt = Optimizer(0)
    try:
        kf, mp, erase, level, stats = call(opt, p)
        q, kf_order, mp_order, e_order = _as_the_member_flattens(p)
        kf2, mp2, erase2, level2, stats2 = call(opt, q)
    finally:
        opt.close()
    assert stats[5] == 2 and erase.any() and level.any()
    # (1) the view-taking form
    assert take(np.float32, 7 * nKF).tobytes() == kf.tobytes() and take(np.float32, 3 * nMP).tobytes() == mp.tobytes()
    assert take(np.uint8, nE).tobytes() == erase.tobytes() and take(np.uint8, nE).tobytes() == level.tobytes() and take(np.int32, 6).tolist() == stats.tolist()
    # (2) the member on the mock map
    pose, nset = take(np.float32, 7 * nKF).reshape(nKF, 7), take(np.int32, nKF)
    pos, nupd = take(np.float32, 3 * nMP).reshape(nMP, 3), take(np.int32, nMP)
    gone, kf_mark, mp_mark = take(np.uint8, nE), take(np.int32, nKF), take(np.int32, nMP)
    assert off == len(raw)
    assert stats2[5] == 2
    free = p["kfFixed"] == 0
    assert pose[kf_order].tobytes() == kf2.tobytes()                      # free keyframes: the entry's output; fixed ones: their input
    assert nset.tolist() == free.astype(int).tolist()
    entered = np.zeros(nMP, bool); entered[mp_order] = True
    assert pos[mp_order].tobytes() == mp2.tobytes() and pos[~entered].tobytes() == p["mpPos"][~entered].tobytes()
    assert nupd.tolist() == entered.astype(int).tolist()
    assert gone[e_order].tobytes() == erase2.tobytes()
    main = 1 + int(np.nonzero(free)[0][0])                                # mpCurrentKF->mnId
    assert (kf_mark == main).all() and (mp_mark[entered] == main).all() and not mp_mark[~entered].any()
