#!/usr/bin/env python3
"""Timing of Optimizer::FullInertialBA over a whole map on MI355X (morb_full_inertial_ba) at N = 500 and 2000 keyframes on the topology of
tools/bench_global_ba.py: keyframes within `reach` 10 (20) of one another share points — the covisibility band — and points seen from the
first and the last reach + 1 keyframes stand for one closed loop; one temporal chain through all keyframes, nothing fixed, as the call
sites have it.  Two calls per size: bInit = 0 with 7 iterations (LoopClosing's) and bInit = 1 with 100 (LocalMapping's; the stop rules end
it long before).  Three runs each (host arrays in, host arrays out, warmed up): the wall clock of the synchronous call and the time per LM
trial; beside them the one-thread CPU oracle (tests/native/full_inertial_ba_oracle.cc) on the same problem, once, and
morb_bundle_adjustment's time per trial on the same visual graph (the camera poses of the same states, the first keyframe fixed): what the
3 x 3 envelope with five block rows per keyframe costs over the 6 x 6 one with one.  The per-kernel split comes from one more run in a
child process under `rocprofv3 --kernel-trace`: kernel time summed by name, per call, grouped into edges (linearize, links, assemble,
errors), Schur (dinv, schur, finish), factor, and back-substitution (backsub, points).  --no-profile leaves the split out; --no-oracle the
oracle; --sizes 500 runs one size.  Prints one JSON line per size and call."""
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES = ((500, 10, 8000), (2000, 20, 20000))      # keyframes, reach, points
CALLS = ((0, 7), (1, 100))                        # bInit, its
RUNS = 3
CHILD_CALLS = 2
GROUPS = {"edges": ("k_fiba_linearize", "k_fiba_links", "k_fiba_assemble", "k_fiba_errors"), "schur": ("k_fiba_dinv", "k_fiba_schur", "k_fiba_finish"),
          "factor": ("k_fiba_factor",), "backsub": ("k_fiba_backsub", "k_fiba_points"), "control": ("k_fiba_setup", "k_fiba_decide")}


def _problem(n, reach, points, init):
    import full_inertial_ba_cases as cases
    from morb_slam_amd.synth import make_full_inertial_ba_problem
    p = make_full_inertial_ba_problem(n, reach, points, 40, seed=5, loop_span=reach + 1, obs_frac=0.6, init=bool(init), n_imu=cases.N_IMU)
    return p, cases.preintegrate(p)


def _call(opt, p, pre, its):
    return opt.FullInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"], pre,
                              p["cam"], p["Tbc12"], its=its, init=p["init"], prior_g=p["priorG"], prior_a=p["priorA"], bias6=p["bias6"])


def _visual_call(opt, p):
    """morb_bundle_adjustment on the same edges: the camera poses of the same states, the first keyframe fixed, no kernel, 10 iterations."""
    from morb_slam_amd.synth import _quat_from_R
    Tbc = np.eye(4); Tbc[:3, :3] = p["Tbc12"][:9].reshape(3, 3); Tbc[:3, 3] = p["Tbc12"][9:]
    Rcb = Tbc[:3, :3].T; tcb = -Rcb @ Tbc[:3, 3]
    pose = np.zeros((len(p["kfState"]), 7), np.float32)
    for k, s in enumerate(p["kfState"].astype(np.float64)):
        Rwb, twb = s[:9].reshape(3, 3), s[9:12]
        pose[k, :4] = _quat_from_R(Rcb @ Rwb.T); pose[k, 4:] = Rcb @ (-Rwb.T @ twb) + tcb
    fixed = np.zeros(len(pose), np.uint8); fixed[0] = 1
    t0 = time.perf_counter()
    _, _, st, _ = opt.BundleAdjustment(pose, fixed, p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"], n_iterations=10, robust=False)
    return (time.perf_counter() - t0) * 1e3, st


def child(n, reach, points, init, its):
    from morb_slam_amd import Optimizer
    opt = Optimizer(0)
    p, pre = _problem(n, reach, points, init)
    for _ in range(CHILD_CALLS):
        _call(opt, p, pre, its)
    opt.close()


def kernel_split(n, reach, points, init, its):
    """Kernel milliseconds per call by group, from a kernel trace of CHILD_CALLS calls; None when the profiler or its database is not there."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    tmp = tempfile.mkdtemp(prefix="bench_fiba_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "-d", tmp, "-o", "fiba", "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(reach),
                            str(points), str(init), str(its)], capture_output=True, text=True, timeout=900)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return None
        con = sqlite3.connect(dbs[0])
        rows = con.execute("select s.kernel_name, sum(d.end - d.start), count(*) from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
                           "group by s.kernel_name").fetchall()
        out = {g: 0.0 for g in GROUPS}
        launches = 0
        for name, ns, count in rows:
            for g, kernels in GROUPS.items():
                if any(k + "E" in name or k + "I" in name for k in kernels):
                    out[g] += ns / 1e6 / CHILD_CALLS
                    launches += count
                    break
        out["launches_per_call"] = launches / CHILD_CALLS
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(profile=True, oracle=True, sizes=None):
    import full_inertial_ba_oracle as fo
    from morb_slam_amd import Optimizer
    fo.lib()              # compiled before any timing
    opt = Optimizer(0)
    for n, reach, points in SIZES:
        if sizes and n not in sizes:
            continue
        for init, its in CALLS:
            p, pre = _problem(n, reach, points, init)
            kf, mp, b6, st, chi = _call(opt, p, pre, its)   # warm-up: the workspace grows here
            wall = []
            for _ in range(RUNS):
                t0 = time.perf_counter(); _call(opt, p, pre, its); wall.append((time.perf_counter() - t0) * 1e3)
            trials = max(int(st[1]), 1)
            res = dict(keyframes=n, reach=reach, bInit=init, its=its, points=len(p["mpPos"]), edges=len(p["eKF"]), links=len(p["iKF1"]), stats4=st.tolist(),
                       chi2=chi.tolist(), wall_ms=wall, per_trial_ms=[w / trials for w in wall])
            if oracle:
                t0 = time.perf_counter(); want = fo.run(p, pre, its=its); oracle_ms = (time.perf_counter() - t0) * 1e3
                res.update(oracle_stats4=want["stats4"].tolist(), oracle_chi2=want["chi2"].tolist(), oracle_ms=oracle_ms,
                           oracle_per_trial_ms=oracle_ms / max(int(want["stats4"][1]), 1))
            if not init:
                _visual_call(opt, p)
                ms, vst = _visual_call(opt, p)
                res.update(visual_ba_ms=ms, visual_ba_stats4=vst.tolist(), visual_ba_per_trial_ms=ms / max(int(vst[1]), 1))
            split = kernel_split(n, reach, points, init, its) if profile else None
            res["kernel_ms_per_call"] = split
            if split:
                res["kernel_ms_per_trial"] = {g: split[g] / trials for g in GROUPS}
                res["factor_us_per_trial_and_block_column"] = split["factor"] / trials / (int(st[2]) // 3) * 1e3
            print(json.dumps(res), flush=True)
    opt.close()


if __name__ == "__main__":
    if len(sys.argv) == 7 and sys.argv[1] == "--child":
        child(*(int(a) for a in sys.argv[2:]))
    else:
        sizes = [int(a) for a in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else None
        main(profile="--no-profile" not in sys.argv, oracle="--no-oracle" not in sys.argv, sizes=sizes)
