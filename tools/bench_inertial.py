#!/usr/bin/env python3
"""Timing of the visual-inertial tracking kernels on MI355X: PreintegrateIMU and PoseInertialOptimizationLastKeyFrame.
--rig: PoseInertialOptimizationLastKeyFrame and LastFrame on the KannalaBrandt8 rig instead (the scene of
tests/test_inertial_gpu.py::test_pose_inertial_optimization_fisheye_rig, LastFrame from LastKeyFrame's own state and prior)."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import imu_calib_diagonals, make_inertial_problem, make_inertial_sequence

dev = torch.device("cuda", 0)
opt = Optimizer(0)
nga, walk = imu_calib_diagonals()


def timed(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


if "--rig" in sys.argv[1:]:
    base = [make_inertial_sequence(500, seed=s, n_imu=20, rig=True) for s in range(4)]
    for F in (4, 64):
        seq = [base[s % 4] for s in range(F)]
        st = lambda i, k: torch.from_numpy(np.stack([p[i][k] for p in seq])).to(dev)
        def pre(i, a, g, d):
            start = torch.from_numpy(np.cumsum([0] + [len(p[i][d]) for p in seq]).astype(np.int32)).to(dev)
            cat = lambda k: torch.from_numpy(np.concatenate([p[i][k] for p in seq])).to(dev)
            out = opt.PreintegrateIMU(start, cat(a), cat(g), cat(d), st(i, "bias"), nga, walk)
            torch.cuda.synchronize()   # (the inputs are temporaries)
            return out
        rig, Tbc = seq[0][0]["rig28"], seq[0][0]["Tbc12"]
        nLeft = torch.tensor([p[0]["Nleft"] for p in seq], dtype=torch.int32, device=dev)
        a = [st(0, k) for k in ("hasMP", "obs", "invSigma2", "Xw", "close", "kfState")] + [pre(0, "acc", "gyro", "dt")]
        b = [st(1, k) for k in ("hasMP", "obs", "invSigma2", "Xw", "close")] + [pre(1, "accF", "gyroF", "dtF"), pre(1, "acc", "gyro", "dt")]
        sA0, sB0 = st(0, "state0"), st(1, "state0")
        stateA = sA0.clone()
        _, _, priorA = opt.PoseInertialOptimizationLastKeyFrame(a[0], a[1], a[2], a[3], a[4], None, Tbc, a[5], a[6], stateA, rig=rig, nLeft=nLeft)
        torch.cuda.synchronize()
        outA = outB = sA = sB = None   # (globals: a call's in/out state lives until the next call replaces it)
        def run_kf():
            global outA, sA
            sA = sA0.clone()
            outA = opt.PoseInertialOptimizationLastKeyFrame(a[0], a[1], a[2], a[3], a[4], None, Tbc, a[5], a[6], sA, rig=rig, nLeft=nLeft, out=outA)
        def run_f():
            global outB, sB
            sB = sB0.clone()
            outB = opt.PoseInertialOptimizationLastFrame(b[0], b[1], b[2], b[3], b[4], None, Tbc, stateA, b[5], b[6], priorA, sB, rig=rig, nLeft=nLeft, out=outB)
        t1, t2 = timed(run_kf), timed(run_f)
        print(f"rig F={F}: PoseInertialOptimizationLastKeyFrame {t1*1e3:.3f} ms/batch, PoseInertialOptimizationLastFrame {t2*1e3:.3f} ms/batch")
    sys.exit(0)

for F in (1, 64, 256):
    probs = [make_inertial_problem(600, seed=s % 16, n_imu=20) for s in range(F)]
    st = lambda k: torch.from_numpy(np.stack([p[k] for p in probs])).to(dev)
    start = torch.from_numpy(np.cumsum([0] + [len(p["dt"]) for p in probs]).astype(np.int32)).to(dev)
    cat = lambda k: torch.from_numpy(np.concatenate([p[k] for p in probs])).to(dev)
    acc, gyro, dt, bias = cat("acc"), cat("gyro"), cat("dt"), st("bias")
    a = [st(k) for k in ("hasMP", "obs", "invSigma2", "Xw", "close", "kfState")]
    s0 = st("state0")
    pre = opt.PreintegrateIMU(start, acc, gyro, dt, bias, nga, walk)
    out = None
    def run():
        global out
        state = s0.clone()
        out = opt.PoseInertialOptimizationLastKeyFrame(a[0], a[1], a[2], a[3], a[4], probs[0]["cam"], probs[0]["Tbc12"], a[5], pre, state, out=out)
    for _ in range(3): run()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): run()
    torch.cuda.synchronize(); t1 = (time.perf_counter() - t0) / 20
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): opt.PreintegrateIMU(start, acc, gyro, dt, bias, nga, walk, out=pre)
    torch.cuda.synchronize(); t2 = (time.perf_counter() - t0) / 20
    print(f"F={F}: PoseInertialOptimizationLastKeyFrame {t1*1e3:.3f} ms/batch ({F/t1:.0f} frames/s), PreintegrateIMU(20 samples) {t2*1e3:.3f} ms/batch")
# CPU oracle for scale
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as orc
p = make_inertial_problem(600, seed=0, n_imu=20)
t0 = time.perf_counter()
for _ in range(20):
    pr = orc.imu_preintegrate(p["bias"], nga, walk, p["acc"], p["gyro"], p["dt"])
    orc.pose_inertial_optimization_last_keyframe(p, pr)
print(f"CPU oracle: {(time.perf_counter()-t0)/20*1e3:.3f} ms/frame (1 core)")
