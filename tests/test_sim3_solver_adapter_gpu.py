"""ORB_SLAM3::Sim3Solver in the reference's signature (include/morb/Sim3Solver.h), driven from C++ with mock keyframes and map points after
srand(seed) (tests/native/sim3_solver_adapter_check.cc): find(), LoopClosing's `while (!bConverge && !bNoMore) iterate(20, ..)` and one
four-argument iterate(20, ..) against the CPU oracle on the same rand() stream — nInliers, vbInliers, bConverge / bNoMore, the returned
matrix and the GetEstimated* bits.  The cases cover pKFm from vpKeyFrameMatchedMP, a rig KF1 (right features' keypoints in mvKeysRight),
negative keyframe indices, bad and missing points, no convergence and N < minInliers."""
import os
import subprocess

import numpy as np
import pytest

import sim3_solver_oracle
from morb_slam_amd.synth import libc_rand, make_sim3_solver_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LEV = ((1.2 ** np.arange(8)) ** 2).astype(np.float32)
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)


def _bits(a):
    a = np.array(a, np.float32, ndmin=1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def _write(path, p, seed, use_kfm, rig1, rng):
    n = p["n"]
    oct1 = np.array([int(np.argmin(np.abs(LEV - s))) for s in p["sigma2_1"]], np.int32)
    oct2 = np.array([int(np.argmin(np.abs(LEV - s))) for s in p["sigma2_2"]], np.int32)
    kfm = (rng.random(n) < 0.5).astype(np.int32) if use_kfm else np.zeros(n, np.int32)
    kind = lambda c: int(c[0] != 0)
    with open(path, "wb") as f:
        f.write(np.array([n, kind(p["cam1"]), kind(p["cam2"]), int(p["fix_scale"]), seed, p["min_inliers"], p["max_iterations"],
                          int(use_kfm), int(rig1)], np.int32).tobytes())
        f.write(np.float64(p["probability"]).tobytes())
        for a in (p["cam1"][1:], p["cam2"][1:], p["T1w"], p["T2w"], LEV):
            f.write(np.asarray(a, np.float32).tobytes())
        for i in range(n):
            f.write(np.uint8(p["entry"][i]).tobytes() + p["Xw1"][i].astype(np.float32).tobytes() + p["Xw2"][i].astype(np.float32).tobytes() +
                    np.array([oct1[i], oct2[i], kfm[i]], np.int32).tobytes())
    q = dict(p)   # what the adapter reads: the level sigma2 of the two keypoints' octaves
    q["sigma2_1"], q["sigma2_2"] = LEV[oct1], LEV[oct2]
    return q


def _read(path, n):
    raw = open(path, "rb").read()
    out, off = [], 0
    for _ in range(3):
        calls, conv, noMore, nIn = np.frombuffer(raw[off:off + 16], np.int32); off += 16
        vb = np.frombuffer(raw[off:off + n], np.uint8); off += n
        fl = np.frombuffer(raw[off:off + 4 * 45], np.float32); off += 4 * 45
        out.append(dict(calls=int(calls), converged=int(conv), noMore=int(noMore), nInliers=int(nIn), mask=vb, ret=fl[:16], T=fl[16:32],
                        R=fl[32:41], t=fl[41:44], s=fl[44]))
    assert off == len(raw)
    return out


def _same_best(a, best, k):
    assert np.array_equal(_bits(a["T"]), _bits(best["bestT12"])), k
    assert np.array_equal(_bits(a["R"]), _bits(best["bestR"])), k
    assert np.array_equal(_bits(a["t"]), _bits(best["bestt"])), k
    assert np.array_equal(_bits(a["s"]), _bits(best["bestScale"])), k


def test_reference_signature_class_on_gpu(tmp_path):
    exe = str(tmp_path / "sim3_solver_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_sim3_solver"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(NATIVE, "sim3_solver_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cases = [(dict(n=300, outlier_frac=0.3), False, False),
             (dict(n=350, outlier_frac=0.6, cam1="kb8", fix_scale=True), True, False),
             (dict(n=320, outlier_frac=0.5, cam2="kb8", neg_idx_frac=0.2, bad_frac=0.1, no_mp1_frac=0.1), True, True),
             (dict(n=400, outlier_frac=0.9), False, True),                                  # no convergence: 15 chunks of 20
             (dict(n=300, outlier_frac=0.2, min_inliers=280), False, False),                 # N < minInliers
             (dict(n=260, outlier_frac=0.75, max_iterations=45, min_inliers=45), True, False),   # converges in the second call
             (dict(n=260, outlier_frac=0.8, max_iterations=45, min_inliers=30), False, True)]    # budget 45 spent in 3 calls
    rng = np.random.default_rng(7)
    seen = {"conv": 0, "noconv": 0, "multi": 0}
    for k, (sp, use_kfm, rig1) in enumerate(cases):
        sp = dict(sp)
        sp.setdefault("min_inliers", 20)
        p = make_sim3_solver_problem(sp.pop("n"), seed=700 + k, **sp)
        seed = 4242 + k
        fin, fout = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
        q = _write(fin, p, seed, use_kfm, rig1, rng)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = _read(fout, p["n"])
        rand = libc_rand(seed, 3 * p["max_iterations"])
        # find(): one call with the whole budget; the four-argument overload returns identity unless it converged
        oc, best = sim3_solver_oracle.run(q, rand)
        o, a = oc[-1], got[0]
        assert (a["converged"], a["noMore"], a["nInliers"]) == (o["converged"], o["noMore"], o["nInliers"]), k
        assert np.array_equal(a["mask"], o["mask"]), k
        assert np.array_equal(_bits(a["ret"]), _bits(o["sim3"] if o["converged"] else IDENTITY)), k
        if o["iterations"] > 0:
            _same_best(a, best, k)
        # the LoopClosing loop: the oracle's calls of 20 until converged or no more
        oc, best = sim3_solver_oracle.run(q, rand, calls=[20] * 1000)
        o, a = oc[-1], got[1]
        assert a["calls"] == len(oc), k
        assert (a["converged"], a["noMore"], a["nInliers"]) == (o["converged"], o["noMore"], o["nInliers"]), k
        assert np.array_equal(a["mask"], o["mask"]), k
        assert np.array_equal(_bits(a["ret"]), _bits(o["sim3"])), k     # bestSim3 (identity where the reference leaves it unset)
        if o["iterations"] > 0:
            _same_best(a, best, k)
        # one iterate(20, bNoMore, vbInliers, nInliers)
        oc, best = sim3_solver_oracle.run(q, rand, calls=[20])
        o, a = oc[-1], got[2]
        assert (a["converged"], a["noMore"], a["nInliers"]) == (o["converged"], o["noMore"], o["nInliers"]), k
        assert np.array_equal(a["mask"], o["mask"]), k
        assert np.array_equal(_bits(a["ret"]), _bits(o["sim3"] if o["converged"] else IDENTITY)), k
        if o["iterations"] > 0:
            _same_best(a, best, k)
        seen["conv" if got[1]["converged"] else "noconv"] += 1
        seen["multi"] += got[1]["calls"] > 1
    assert seen["conv"] >= 3 and seen["noconv"] >= 2 and seen["multi"] >= 2, seen
