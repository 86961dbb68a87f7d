"""ORB_SLAM3::TwoViewReconstruction in the reference's signature (include/morb/TwoViewReconstruction.h), driven from C++ with mock
keypoints, SE3f and Point3f (tests/native/two_view_adapter_check.cc): one reconstructor, Reconstruct on three corpus problems in one
process.  The class seeds rand() once (srand(0), after the device has started) and draws 8 * iterations values per call, so call k
must equal the CPU oracle fed values [1600 k, 1600 (k + 1)) of libc's stream after srand(0), and the next rand() value after the
calls must be the stream's next one: a stream that moved fails by itself."""
import os
import subprocess

import numpy as np
import pytest

import two_view_corpus
import two_view_oracle
from morb_slam_amd.synth import libc_rand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
PICK = (0, 12, 20)   # a general scene (F), a corner scene (H), a small baseline (fails on parallax)


def test_reference_signature_class_on_gpu(tmp_path):
    exe = str(tmp_path / "two_view_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_two_view"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(NATIVE, "two_view_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    probs, _ = two_view_corpus.problems()
    probs = [probs[k] for k in PICK]
    its = 200
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(probs)).tobytes() + probs[0]["K4"].astype(np.float32).tobytes() + np.float32(1.0).tobytes() + np.int32(its).tobytes())
        for p in probs:
            f.write(np.array([p["n1"], p["n2"]], np.int32).tobytes() + p["kp1"].tobytes() + p["kp2"].tobytes() + p["matches12"].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    stream = libc_rand(0, 8 * its * len(probs) + 1)
    off, oks = 0, []
    for k, p in enumerate(probs):
        n1 = p["n1"]
        ok, nP, nT = np.frombuffer(raw[off:off + 12], np.int32); off += 12
        T = np.frombuffer(raw[off:off + 48], np.float32); off += 48
        P = np.frombuffer(raw[off:off + 12 * n1], np.float32).reshape(n1, 3); off += 12 * n1
        tri = np.frombuffer(raw[off:off + n1], np.uint8); off += n1
        o = two_view_oracle.run(dict(p, max_iterations=its, sigma=1.0), stream[8 * its * k:8 * its * (k + 1)])
        assert int(ok) == o["ok"], k
        oks.append(int(ok))
        if not o["ok"]:
            assert (nP, nT) == (3, 2), k   # a false return leaves the caller's vectors alone
            continue
        assert (nP, nT) == (n1, n1), k
        assert np.abs(T - o["T21"]).max() <= 1e-4 and np.array_equal(tri, o["triangulated"]), k
        assert (np.linalg.norm(P - o["P3D"], axis=1) / np.maximum(1.0, np.linalg.norm(o["P3D"], axis=1))).max() <= 1e-4, k
    marker = int(np.frombuffer(raw[off:off + 4], np.int32)[0])
    assert off + 4 == len(raw) and marker == int(stream[8 * its * len(probs)])
    assert oks == [1, 1, 0]
