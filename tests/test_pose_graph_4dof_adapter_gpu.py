"""Optimizer::OptimizeEssentialGraph4DoF(PoseGraph4DoFView&) (include/morb/Optimizer.h), driven from C++
(tests/native/pose_graph_4dof_adapter_check.cc): the view call gives the bytes of the C entry called from Python on the same problem; and
the reference-typed member on a mock map (tests/native/pose_graph_4dof_member_check.cc) writes back the bytes the C entry gives on the
problem the member flattens."""
import os
import subprocess

import numpy as np
import pytest

import pose_graph_4dof_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", *extra, "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(NATIVE, name + ".cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("name", ["band8", "several_fixed"])
def test_view_call_equals_the_c_entry(tmp_path, name):
    from morb_slam_amd import Optimizer
    exe = _build(tmp_path, "pose_graph_4dof_adapter_check")
    p = cases.case_problem(name)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(cases.problem_bytes(p))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    opt = Optimizer(0)
    try:
        P, mp, stats, chi2 = opt.OptimizeEssentialGraph4DoF(p["kfPose"], p["kfBody"], p["kfFixed"], p["Tcb12"], p["eI"], p["eJ"], p["eTij"], p["mpPos"], p["mpRef"], p["kfScw"])
    finally:
        opt.close()
    assert stats[0] > 0 and np.abs(P - p["kfPose"]).max() > 1e-3
    assert open(fout, "rb").read() == P.tobytes() + mp.tobytes() + stats.tobytes() + chi2.tobytes()


def _quat_of(R):
    """Eigen::Quaterniond(Matrix3d), normalised: x y z w."""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        q[:3] = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (0.5 / t)
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        q[3] = (R[k, j] - R[j, k]) * (0.5 / t)
        q[j] = (R[j, i] + R[i, j]) * (0.5 / t)
        q[k] = (R[k, i] + R[i, k]) * (0.5 / t)
    return q / np.sqrt((q * q).sum())


def test_member_on_a_mock_map_equals_the_c_entry(tmp_path):
    """The program dumps the graph the member flattens from its mock map (checked against a hand-written expectation in the CPU suite), runs
    the member on the library, and dumps the map: every keyframe with a vertex holds SetPose(the unit quaternion of Rcw, tcw, as floats) of
    the C entry's result, the bad keyframe its old pose; every point whose reference keyframe has a vertex holds the C entry's corrected
    position."""
    from morb_slam_amd import Optimizer
    exe = _build(tmp_path, "pose_graph_4dof_member_check", ["-I" + os.path.join(NATIVE, "mock_pose_graph_4dof")])
    fprob, fres = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    r = subprocess.run([exe, fprob, fres], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fprob, "rb").read()
    nKF, nE, nMP = np.frombuffer(raw, np.int32, 3)
    assert (nKF, nE, nMP) == (6, 12, 5)
    off = 12

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    P0, B0, fx, tcb = take(np.float64, 12 * nKF).reshape(nKF, 12), take(np.float64, 12 * nKF).reshape(nKF, 12), take(np.uint8, nKF), take(np.float32, 12)
    eI, eJ, M = take(np.int32, nE), take(np.int32, nE), take(np.float64, 12 * nE).reshape(nE, 12)
    mp0, ref, scw = take(np.float32, 3 * nMP).reshape(nMP, 3), take(np.int32, nMP), take(np.float64, 8 * nKF).reshape(nKF, 8)
    assert off == len(raw)
    opt = Optimizer(0)
    try:
        P, mp, stats, chi2 = opt.OptimizeEssentialGraph4DoF(P0, B0, fx, tcb, eI, eJ, M, mp0, ref, scw)
    finally:
        opt.close()
    assert stats[0] > 0 and stats[2] == 5 and chi2[1] < chi2[0]
    res = open(fres, "rb").read()
    pose = np.frombuffer(res, np.float32, 49).reshape(7, 7)
    pos = np.frombuffer(res, np.float32, 15, 49 * 4).reshape(5, 3)
    nset = np.frombuffer(res, np.int32, 7, 64 * 4)
    assert nset.tolist() == [1, 1, 1, 0, 1, 1, 1]
    rows = [0, 1, 2, 4, 5, 6]                    # keyframe of vertex v (k3 is bad)
    want = np.array([np.concatenate([_quat_of(P[v, :9].reshape(3, 3)), P[v, 9:]]) for v in range(nKF)]).astype(np.float32)
    assert np.abs(pose[rows] - want).max() <= 1e-6   # (numpy's sqrt and divisions against the program's: a float ulp of a unit quaternion)
    assert pose[rows][:, 4:].tobytes() == P[:, 9:].astype(np.float32).tobytes()
    assert np.abs(P[5, 9:] - P0[5, 9:]).max() > 1e-3          # (the current keyframe moved)
    assert pos[ref >= 0].tobytes() == mp[ref >= 0].tobytes() and np.abs(pos[1] - mp0[1]).max() > 1e-4
    assert pos[2].tobytes() == np.array([3.0, 1.0, 3.4], np.float32).tobytes()   # the bad point keeps its position
    assert pos[4].tobytes() == mp0[4].tobytes() and ref[4] == -1                 # ... and so does the point whose reference keyframe is bad
