"""Optimizer::OptimizeEssentialGraph(MergeEssentialGraphView&) (include/morb/Optimizer.h), driven from C++
(tests/native/merge_graph_adapter_check.cc): the view call gives the bytes of the C entry called from Python on the same problem; and the
reference-typed member of overload 2 on a mock map (tests/native/merge_graph_member_check.cc) leaves poses, both BefMerge members and
points equal to the C entry's result on the problem the member flattens."""
import os
import subprocess

import numpy as np
import pytest

import merge_graph_cases as cases
import merge_graph_oracle as mo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _build(tmp_path, name, mocks=False):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + (["-I" + os.path.join(NATIVE, "mock_merge_graph")] if mocks else []) +
                          ["-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(NATIVE, name + ".cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _entry(p):
    from morb_slam_amd import Optimizer
    opt = Optimizer(0)
    try:
        return opt.OptimizeEssentialGraphMerge(p["kfLists"], *[p[k] for k in mo.POSES], p["cI"], p["cJ"], p["mpPos"], p["mpRef"])
    finally:
        opt.close()


@pytest.mark.parametrize("name", ["merge", "disjoint"])
def test_view_call_equals_the_c_entry(tmp_path, name):
    exe = _build(tmp_path, "merge_graph_adapter_check")
    p = cases.case_problem(name)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(cases.problem_bytes(p))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _entry(p)
    assert got["stats4"][0] > 0 and np.abs(got["kfTcw"] - p["kfTcw"]).max() > 1e-3
    assert open(fout, "rb").read() == b"".join(got[k].tobytes() for k in mo.POSES + ("mpPos", "cKept", "stats4", "chi2"))


def test_member_on_a_mock_map_equals_the_c_entry(tmp_path):
    """The program dumps the problem the member flattens from its mock map (checked against a hand-written expectation in the CPU suite), runs
    the member on the library, and dumps the map.  Every non-bad keyframe of vpNonFixedKFs — k6 and k7, which are also in the window,
    included — holds the C entry's Tcw and, in its BefMerge members, the entry's Tcw / Twc at entry; the bad keyframe, the merged map's and
    the unlisted ones hold what they held.  Points with a bad-flagged reference hold the C entry's position; the point whose reference is
    in vpFixedKFs, the bad one and those without a usable reference keep theirs."""
    exe = _build(tmp_path, "merge_graph_member_check", mocks=True)
    fprob, fres = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    r = subprocess.run([exe, fprob, fres], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fprob, "rb").read()
    nKF, nC, nMP = (int(x) for x in np.frombuffer(raw, np.int32, 3))
    assert (nKF, nC, nMP) == (7, 19, 8)
    off = 12

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    p = dict(kfLists=take(np.uint8, nKF))
    for k in mo.POSES:
        p[k] = take(np.float32, 7 * nKF).reshape(nKF, 7)
    p.update(cI=take(np.int32, nC), cJ=take(np.int32, nC), mpPos=take(np.float32, 3 * nMP).reshape(nMP, 3), mpRef=take(np.int32, nMP))
    assert off == len(raw) and p["kfLists"].tolist() == [1, 1, 4, 4, 4, 6, 6] and p["mpRef"].tolist() == [3, 4, -1, 0, 5, -1, -1, -1]
    got = _entry(p)
    assert got["stats4"][0] > 0 and got["stats4"][2] == 3 and got["chi2"][1] < got["chi2"][0] and got["cKept"].tolist() == [1] * 8 + [0] + [1] * 10
    res = open(fres, "rb").read()
    kf = np.frombuffer(res, np.float32, 10 * 21).reshape(10, 3, 7)          # per keyframe: mTcw, mTcwBefMerge, mTwcBefMerge
    pos = np.frombuffer(res, np.float32, 24, 10 * 21 * 4).reshape(8, 3)
    nset = np.frombuffer(res, np.int32, 10, (10 * 21 + 24) * 4)
    assert nset.tolist() == [0, 0, 1, 1, 0, 1, 1, 1, 0, 0]
    row = {2: 2, 3: 3, 5: 4, 6: 5, 7: 6}                                     # keyframe -> vertex (k4 is bad)
    for k, v in row.items():
        assert kf[k, 0].tobytes() == got["kfTcw"][v].tobytes(), k
        assert kf[k, 1].tobytes() == got["kfTcwBefMerge"][v].tobytes() == p["kfTcw"][v].tobytes(), k
        assert kf[k, 2].tobytes() == got["kfTwcBefMerge"][v].tobytes() == p["kfTwc"][v].tobytes(), k
    for k, v in ((0, 0), (1, 1)):                                            # the merged map's keyframes keep everything
        assert kf[k, 0].tobytes() == p["kfTcw"][v].tobytes() and kf[k, 1].tobytes() == p["kfTcwBefMerge"][v].tobytes()
    assert np.abs(kf[3, 0, 4:] - p["kfTcw"][3, 4:]).max() > 1e-3           # (a free keyframe moved)
    assert np.abs(kf[6, 0] - p["kfTcw"][5]).max() < 1e-6                    # (an overlapped one made the round trip only)
    moved = [0, 1, 4]
    assert pos[moved].tobytes() == got["mpPos"][moved].tobytes() and np.abs(pos[0] - p["mpPos"][0]).max() > 1e-4
    assert pos[3].tobytes() == got["mpPos"][3].tobytes()                     # reference in vpFixedKFs: as the C entry, and as it was (below)
    for j in (2, 3, 5, 6, 7):
        assert pos[j].tobytes() == np.array([1.0 + j, 0.5 * j, np.float32(4.0) - np.float32(0.3) * np.float32(j)], np.float32).tobytes(), j
