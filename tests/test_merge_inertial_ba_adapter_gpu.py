"""Optimizer::MergeInertialBA(MergeInertialBAView&, bool*) and the reference-typed MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap,
corrPoses) (include/morb/Optimizer.h), driven from C++ (tests/native/merge_inertial_ba_adapter_check.cc): the view call gives the bytes of
the C entry called from Python on the same problem, with the stop flag clear and set, and the mock-map member — which selects its windows and
covisible keyframes itself and takes vertices, points and edges in its own order — the bytes of the C entry on the problem flattened that way:
poses through Tcw = (Rcb Rwb^T, tcb - Rcb Rwb^T twb), velocities, biases, points, the erase list and corrPoses."""
import os
import subprocess

import numpy as np
import pytest

import merge_inertial_ba_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("name", ["mix-3x1-s0", "kb8-9x5-s0"])
def test_view_call_and_member_equal_the_c_entry(tmp_path, name):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "merge_inertial_ba_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_merge_inertial_ba"), "-I" + os.path.join(NATIVE, "mock_ref"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "merge_inertial_ba_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p, pre = cases.problem(name)
    nKF, nMP, nE, nI = len(p["kfState"]), len(p["mpPos"]), len(p["eKF"]), len(p["iKF1"])
    rig = p["rig28"] is not None
    c = p["cam"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        nA = int(np.where(p["kfKind"] == 1)[0][0])                       # chain A = [0, nA), chain B = the fixed keyframe and the free ones behind it
        nB = 1 + int((p["kfKind"][nA:] == 0).sum())
        f.write(np.array([nKF, nMP, nE, nI, rig, nA, nB], np.int32).tobytes() + f32([c["fx"], c["fy"], c["cx"], c["cy"], c["bf"]]) +
                f32(p["rig28"] if rig else np.zeros(28)) + f32(p["Tbc12"]) + f32(p["kfState"]) + p["kfKind"].astype(np.uint8).tobytes() + f32(p["mpPos"]) +
                p["eKF"].astype(np.int32).tobytes() + p["eMP"].astype(np.int32).tobytes() + f32(p["eObs"]) + f32(p["eInvSigma2"]) +
                p["iKF1"].astype(np.int32).tobytes() + p["iKF2"].astype(np.int32).tobytes() + f32(pre))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "merge inertial ba adapter ok" in r.stdout, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    opt = Optimizer(0)
    try:
        for stop in (0, 1):
            kf, mp, erase, stats = opt.MergeInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"],
                                                       p["iKF2"], pre, p["cam"], p["Tbc12"], stop_flag=np.array([stop], np.uint8), rig=p["rig28"])
            assert stats[2] == 1 - stop and (erase.any() or stop)
            assert take(np.float32, 21 * nKF).tobytes() == kf.tobytes() and take(np.float32, 3 * nMP).tobytes() == mp.tobytes()
            assert take(np.uint8, nE).tobytes() == erase.tobytes() and take(np.int32, 3).tolist() == stats.tolist()
        # (2) the member on the mock map.  It reads keyframe states in the order of its vertices and point positions in the order of its points
        rec = np.dtype([("n", np.int32, 5), ("R", np.float32, 9), ("t", np.float32, 3), ("v", np.float32, 3), ("b", np.float32, 6), ("S", np.float64, 8)])
        K = take(np.uint8, rec.itemsize * nKF).view(rec)
        prec = np.dtype([("n", np.int32, 2), ("X", np.float32, 3)])
        M = take(np.uint8, prec.itemsize * nMP).view(prec)
        gone, nbias, changes = take(np.uint8, nE), take(np.int32, nI), take(np.int32, 1)[0]
        assert off == len(raw)
        q, kf_order, mp_order, e_order, l_order = _as_the_member_flattens(p, pre, K["n"][:, 0], M["n"][:, 0], nA, nB)
        kf2, mp2, erase2, stats2 = opt.MergeInertialBA(q["kfState"], q["kfKind"], q["mpPos"], q["eKF"], q["eMP"], q["eObs"], q["eInvSigma2"], q["iKF1"],
                                                       q["iKF2"], q["pre"], p["cam"], p["Tbc12"], rig=p["rig28"])
    finally:
        opt.close()
    kind = p["kfKind"]
    assert stats2[2] == 1 and erase2.any() and changes == 1
    assert set(np.where(kind != 3)[0]) <= set(kf_order) and (kind[kf_order] == 3).any() and len(l_order) == nI   # both chains enter whole
    Tbc = np.ascontiguousarray(p["Tbc12"], np.float32).astype(np.float64)
    for row, k in enumerate(kf_order):
        free, free15 = kind[k] in (0, 3), kind[k] == 0
        assert K["n"][k][1:].tolist() == [int(free), int(free15), int(free15), int(free)], (k, K["n"][k])
        if not free:
            continue
        st = kf2[row].astype(np.float64)
        Rcw, tcw = np.zeros(9), np.zeros(3)          # the member's own sums, term by term
        for r in range(3):
            for c in range(3):
                a = 0.0
                for i in range(3):
                    a += Tbc[3 * i + r] * st[3 * c + i]
                Rcw[3 * r + c] = a
        for r in range(3):
            a = 0.0
            for i in range(3):
                a -= Tbc[3 * i + r] * Tbc[9 + i]
            for c in range(3):
                a -= Rcw[3 * r + c] * st[9 + c]
            tcw[r] = a
        assert K["R"][k].tobytes() == Rcw.astype(np.float32).tobytes() and K["t"][k].tobytes() == tcw.astype(np.float32).tobytes(), k
        assert K["S"][k].tolist() == [0, 0, 0, 1] + tcw.astype(np.float32).astype(np.float64).tolist() + [1.0]      # corrPoses: the float pose, scale 1
        want_vb = kf2[row][12:] if free15 else p["kfState"][k][12:]
        assert np.concatenate([K["v"][k], K["b"][k]]).tobytes() == np.ascontiguousarray(want_vb, np.float32).tobytes(), k
    out_of_graph = [k for k in range(nKF) if k not in kf_order]
    for k in out_of_graph:
        assert K["n"][k].tolist() == [-1, 0, 0, 0, 0]
    entered = np.zeros(nMP, bool); entered[mp_order] = True
    assert M["X"][mp_order].tobytes() == mp2.tobytes() and M["X"][~entered].tobytes() == np.ascontiguousarray(p["mpPos"], np.float32)[~entered].tobytes()
    assert M["n"][:, 1].tolist() == entered.astype(int).tolist()
    in_graph = np.zeros(nE, bool); in_graph[e_order] = True
    assert gone[e_order].tobytes() == erase2.tobytes() and not gone[~in_graph].any()
    assert nbias.tolist() == [1] * nI


def _as_the_member_flattens(p, pre, kf_read, mp_read, nA, nB):
    """The problem in the member's order: keyframes and points in the order the member read them (the mock map notes it; -1: not in the graph),
    edges by point with a point's observations by keyframe, links in the order of the windows (each keyframe of vpOptimizableKFs with its
    predecessor).  Returns (problem, keyframe order, point order, edge order, link order)."""
    kf_order = [int(k) for k in np.argsort(kf_read, kind="stable") if kf_read[k] >= 0]
    mp_order = [int(j) for j in np.argsort(mp_read, kind="stable") if mp_read[j] >= 0]
    kf_new = {k: i for i, k in enumerate(kf_order)}
    mp_new = {j: i for i, j in enumerate(mp_order)}
    e_order = sorted((e for e in range(len(p["eKF"])) if int(p["eKF"][e]) in kf_new and int(p["eMP"][e]) in mp_new),
                     key=lambda e: (mp_new[int(p["eMP"][e])], int(p["eKF"][e]), e))
    link_of = {int(k2): i for i, k2 in enumerate(p["iKF2"])}
    l_order = [link_of[k] for k in kf_order if k in link_of and (0 < k < nA or nA < k < nA + nB)]
    q = dict(kfState=p["kfState"][kf_order], kfKind=p["kfKind"][kf_order], mpPos=p["mpPos"][mp_order],
             eKF=np.array([kf_new[int(p["eKF"][e])] for e in e_order], np.int32), eMP=np.array([mp_new[int(p["eMP"][e])] for e in e_order], np.int32),
             eObs=p["eObs"][e_order], eInvSigma2=p["eInvSigma2"][e_order],
             iKF1=np.array([kf_new[int(p["iKF1"][i])] for i in l_order], np.int32), iKF2=np.array([kf_new[int(p["iKF2"][i])] for i in l_order], np.int32),
             pre=np.ascontiguousarray(pre, np.float32)[l_order])
    return q, kf_order, mp_order, e_order, l_order
