"""Optimizer::BundleAdjustment(InitialMapView&) / CreateInitialMapMonocular(InitialMapView&) and the reference-typed GlobalBundleAdjustemnt
(include/morb/Optimizer.h), driven from C++ (tests/native/initial_map_adapter_check.cc): the view call equals the C entry called from
Python on the same problem bit for bit, and the reference signature writes back what the bare bundle adjustment gives, for both nLoopKF
cases."""
import os
import subprocess

import numpy as np
import pytest

from morb_slam_amd.synth import initial_map_frame_params, make_initial_map_problem, pack_initial_map_problems

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _entry(opt, p, **kw):
    t = pack_initial_map_problems([p], torch.device("cuda", 0))
    out = opt.CreateInitialMapMonocular(initial_map_frame_params(p), t["img1"], t["img2"], t["count"], t["kps"], t["matches12"], t["ok"], t["T21"], t["P3D"],
                                        t["triangulated"], cam8=p["cam8"], kb8=p["kb8"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[0] for k, v in out.items()}


@pytest.mark.parametrize("cam", ["pinhole", "kb8"])
def test_view_call_equals_the_c_entry(tmp_path, cam):
    from morb_slam_amd import Optimizer
    exe = str(tmp_path / "initial_map_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_initial_map"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "initial_map_adapter_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p = make_initial_map_problem(seed=90, n_points=140, cam=cam, baseline=1.0 if cam == "kb8" else 0.4)
    n1, n2 = p["n1"], p["n2"]
    pad = lambda a: np.concatenate([a, np.zeros(16 - len(a), np.float32)]).astype(np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n1, n2, p["nlevels"], p["kb8"]], np.int32).tobytes() + p["cam8"].tobytes() + pad(p["scaleFactors"]).tobytes() +
                pad(p["levelSigma2"]).tobytes() + p["T21"].tobytes() + p["kp1"].tobytes() + p["kp2"].tobytes() + p["matches12"].tobytes() +
                p["triangulated"].tobytes() + p["P3D"].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(raw, dt, n, off)
        off += a.nbytes
        return a

    def view():
        head, T, chi2, med = take(np.int32, 5), take(np.float32, 12), take(np.float64, 2), take(np.float32, 1)
        return dict(head=head, Tcw2=T, chi2=chi2, median=med, mpPos=take(np.float32, 3 * n1), mpNormal=take(np.float32, 3 * n1),
                    mpDist=take(np.float32, 2 * n1), hasMP=take(np.uint8, n1))

    opt = Optimizer(0)
    try:
        for kw, extra in ((dict(nIterations=10, robust=False, depthScale=0.0, minTracked=0), False), (dict(nIterations=20, robust=True, depthScale=4.0, minTracked=50), True)):
            a, e = view(), _entry(opt, p, **kw)
            assert a["head"].tolist() == [int(e["status"])] + e["stats"].tolist(), (a["head"], e["status"], e["stats"])
            assert a["Tcw2"].tobytes() == e["Tcw2"].tobytes() and a["chi2"].tobytes() == e["chi2"].tobytes() and a["median"][0] == e["median"]
            for k in ("mpPos", "mpNormal", "mpDist", "hasMP"):
                assert a[k].tobytes() == e[k][:n1].tobytes(), k
            if extra:
                assert take(np.int32, 1)[0] == 1 and a["head"][0] == 1
        bare = _entry(opt, p, nIterations=20, robust=True, depthScale=0.0, minTracked=0)
    finally:
        opt.close()
    has = bare["hasMP"][:n1] != 0
    for loopKF in (0, 7):
        T, pos, upd, marks = take(np.float32, 12), take(np.float32, 3 * n1).reshape(n1, 3), take(np.int32, n1), take(np.int32, 2)
        assert np.abs(T - bare["Tcw2"]).max() <= 1e-6, loopKF      # (the mock SE3f keeps the matrix it is given)
        assert pos[has].tobytes() == bare["mpPos"][:n1][has].tobytes() and not pos[~has].any(), loopKF
        assert np.array_equal(upd[has], np.full(has.sum(), 100 if loopKF == 0 else 7)) and not upd[~has].any(), loopKF
        assert marks.tolist() == ([0, 0] if loopKF == 0 else [7, 7])
    assert off == len(raw)
