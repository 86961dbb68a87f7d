"""Optimizer::OptimizeEssentialGraph(EssentialGraphView&) (include/morb/Optimizer.h), driven from C++
(tests/native/essential_graph_adapter_check.cc): the view call gives the bytes of the C entry called from Python on the same problem; and
the reference-typed member of overload 1 on a mock map (tests/native/essential_graph_member_check.cc) writes back the bytes the C entry
gives on the problem the member flattens."""
import os
import subprocess

import numpy as np
import pytest

import essential_graph_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("name", ["band8", "several_fixed"])
def test_view_call_equals_the_c_entry(tmp_path, name):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "essential_graph_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(NATIVE, "essential_graph_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p = cases.case_problem(name)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(cases.problem_bytes(p))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    opt = Optimizer(0)
    try:
        S, mp, stats, chi2 = opt.OptimizeEssentialGraph(p["kfSim3"], p["kfFlags"], p["eI"], p["eJ"], p["eSji"], p["mpPos"], p["mpRef"])
    finally:
        opt.close()
    assert stats[0] > 0 and np.abs(S - p["kfSim3"]).max() > 1e-3
    assert open(fout, "rb").read() == S.tobytes() + mp.tobytes() + stats.tobytes() + chi2.tobytes()


def test_member_on_a_mock_map_equals_the_c_entry(tmp_path):
    """The program dumps the graph the member flattens from its mock map (checked against a hand-written expectation in the CPU suite), runs
    the member on the library, and dumps the map: every keyframe with a vertex holds SetPose(q as float, t as float / s as float) of the C
    entry's estimate, the bad keyframe its old pose; every point with a reference holds the C entry's corrected position."""
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "essential_graph_member_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_essential_graph"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(NATIVE, "essential_graph_member_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fprob, fres = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    r = subprocess.run([exe, fprob, fres], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fprob, "rb").read()
    nKF, nE, nMP = np.frombuffer(raw, np.int32, 3)
    assert (nKF, nE, nMP) == (6, 14, 5)
    off = 12

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    S0, fl, eI, eJ = take(np.float64, 8 * nKF).reshape(nKF, 8), take(np.uint8, nKF), take(np.int32, nE), take(np.int32, nE)
    M, mp0, ref = take(np.float64, 8 * nE).reshape(nE, 8), take(np.float32, 3 * nMP).reshape(nMP, 3), take(np.int32, nMP)
    assert off == len(raw)
    opt = Optimizer(0)
    try:
        S, mp, stats, chi2 = opt.OptimizeEssentialGraph(S0, fl, eI, eJ, M, mp0, ref)
    finally:
        opt.close()
    assert stats[0] > 0 and stats[2] == 5 and chi2[1] < chi2[0]
    res = open(fres, "rb").read()
    pose = np.frombuffer(res, np.float32, 49).reshape(7, 7)
    pos = np.frombuffer(res, np.float32, 15, 49 * 4).reshape(5, 3)
    nset = np.frombuffer(res, np.int32, 7, 64 * 4)
    assert nset.tolist() == [1, 1, 1, 0, 1, 1, 1]
    rows = [0, 1, 2, 4, 5, 6]                    # keyframe of vertex v (k3 is bad)
    want = np.concatenate([S[:, :4].astype(np.float32), S[:, 4:7].astype(np.float32) / S[:, 7:8].astype(np.float32)], 1)
    assert pose[rows].tobytes() == want.tobytes()
    assert np.abs(pose[6, 4:] - S0[5, 4:7] / S0[5, 7]).max() > 1e-3          # (the current keyframe moved)
    assert pos[ref >= 0].tobytes() == mp[ref >= 0].tobytes() and np.abs(pos[1] - mp0[1]).max() > 1e-4
    assert pos[2].tobytes() == np.array([3.0, 1.0, 3.4], np.float32).tobytes()   # the bad point keeps its position
