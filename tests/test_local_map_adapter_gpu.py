"""ORB_SLAM3::Tracking::UpdateLocalMap() with the reference's member names (include/morb/Tracking.h), driven from C++ on mock Frame /
KeyFrame / MapPoint / Atlas types (tests/native/local_map_adapter_check.cc, tests/native/mock_tracking): the member flattens the map
from the pointers, runs the GPU entry and writes back.  Both vectors, pKFmax on the tracker and on the frame, the NULLed entries of the
voting frame, the untouched other frame and both sets of stamps must equal the CPU oracle on the same map."""
import os
import subprocess

import numpy as np
import pytest

import local_map_corpus as corpus
import local_map_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
FRAME_ID = 100


def _write(path, s, q, inertial, imu_initialized, last_reloc, other_frame):
    """The voting frame is the scene's frame q: the current frame unless the IMU is initialised and the relocalisation is old."""
    nkf, nmp = s["nkf"], s["nmp"]
    order = np.arange(nkf) if s["kfOrder"] is None else s["kfOrder"]
    lines = [f"{nkf} {nmp} {4 if inertial else 1} {int(imu_initialized)} {FRAME_ID} {last_reloc} {int(s['lastKf'][q])}"]
    for k in range(nkf):
        cov = [int(c) for c in s["covis"][k] if c >= 0]
        row = s["kfMp"][k, :s["kfCount"][k]].tolist()
        lines.append(" ".join(map(str, [int(order[k]), int(s["kfFlags"][k] & 1), int(s["parent"][k]), int(s["prevKf"][k]), len(cov), *cov, len(row), *row])))
    for m in range(nmp):
        obs = s["mpObsKf"][s["mpObsStart"][m]:s["mpObsStart"][m + 1]].tolist()
        lines.append(" ".join(map(str, [int(s["mpFlags"][m] & 1), len(obs), *obs])))
    voting = s["frameMp"][q, :s["count"][q]].tolist()
    uses_last = imu_initialized and not FRAME_ID < last_reloc + 2
    cur, last = (other_frame, voting) if uses_last else (voting, other_frame)
    lines += [" ".join(map(str, [len(cur), *cur])), " ".join(map(str, [len(last), *last]))]
    open(path, "w").write("\n".join(lines) + "\n")
    return uses_last


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("local_map_adapter") / "local_map_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_tracking"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", out, os.path.join(NATIVE, "local_map_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("name,q,imu_initialized,last_reloc", [("base", 1, False, 0), ("base_inertial", 0, True, 0), ("base_inertial", 2, True, FRAME_ID - 1),
                                                               ("bad_parent_added", 0, False, 0)])
def test_reference_member_on_gpu(exe, tmp_path, name, q, imu_initialized, last_reloc):
    s, inertial = corpus.get(name)
    bad = np.flatnonzero(s["mpFlags"] & 1)
    other = [int(bad[0]) if len(bad) else 0, -1, 1]          # the frame that does not vote keeps its entries, a bad point included
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    uses_last = _write(fin, s, q, inertial, imu_initialized, last_reloc, other)
    assert uses_last == (imu_initialized and last_reloc == 0)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {ln.split()[0]: [int(x) for x in ln.split()[2:]] if ln.split()[0] != "R" else int(ln.split()[1]) for ln in open(fout).read().strip().split("\n")}
    want = oracle.update(s, q, inertial)
    assert got["K"] == want["localKf"].tolist() and got["R"] == want["refKf"] and got["P"] == want["localMp"].tolist()
    voting = want["frameMp"][:s["count"][q]].tolist()
    assert got["L" if uses_last else "C"] == voting and got["C" if uses_last else "L"] == other
    assert got["SK"] == sorted(want["localKf"].tolist()) and got["SP"] == sorted(want["localMp"].tolist())
    assert len(got["K"]) >= 2 and len(got["P"]) >= 4
    if name != "bad_parent_added":
        assert voting != s["frameMp"][q, :s["count"][q]].tolist()     # a bad point was NULLed
