#!/usr/bin/env python3
"""Timing of Optimizer::BundleAdjustment over a whole map on MI355X (morb_bundle_adjustment) at N = 500 and 2000 keyframes on the topology of
tools/bench_essential_graph.py and tools/bench_pose_graph_4dof.py with points added: keyframes within `reach` 10 (20) of one another share
points — the covisibility band — and points seen from the first and the last reach + 1 keyframes stand for one closed loop (that many long
rows).  Pinhole, monocular and stereo observations, no robust kernel, ten iterations: LoopClosing's call.  Three runs (host arrays in, host
arrays out, warmed up): the wall clock of the synchronous call and the time per LM trial; beside them the one-thread CPU oracle
(tests/native/global_ba_oracle.cc) on the same problem, once.  The per-kernel split comes from one more run in a child process under
`rocprofv3 --kernel-trace`: kernel time summed by name, per call, grouped into edges (linearize, assemble, errors), Schur (dinv, schur,
schur_finish), factor, and back-substitution (backsub, points); the factor's time per trial and block column stands beside the 7 x 7 and
4 x 4 kernels' figures of profiles/r17 and profiles/r18.  --no-profile leaves the split out.  Prints one JSON line per size."""
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
RUNS = 3
CHILD_CALLS = 2
GROUPS = {"edges": ("k_gba_linearize", "k_gba_assemble", "k_gba_errors"), "schur": ("k_gba_dinv", "k_gba_schur"), "factor": ("k_gba_factor",),
          "backsub": ("k_gba_backsub", "k_gba_points"), "control": ("k_gba_maxdiag", "k_gba_decide")}


def _problem(n, reach, points):
    from morb_slam_amd.synth import make_global_ba_problem
    return make_global_ba_problem(n, reach, points, 40, seed=5, loop_span=reach + 1, obs_frac=0.6)


def _call(opt, p):
    return opt.BundleAdjustment(p["kfPose"], p["kfFixed"], p["mpPos"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["cam"], n_iterations=10, robust=False)


def child(n, reach, points):
    from morb_slam_amd import Optimizer
    opt, p = Optimizer(0), _problem(n, reach, points)
    for _ in range(CHILD_CALLS):
        _call(opt, p)
    opt.close()


def kernel_split(n, reach, points):
    """Kernel milliseconds per call by group, from a kernel trace of CHILD_CALLS calls; None when the profiler or its database is not there."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    tmp = tempfile.mkdtemp(prefix="bench_gba_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "-d", tmp, "-o", "gba", "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(reach),
                            str(points)], capture_output=True, text=True, timeout=900)
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
                if any(k + "E" in name or k + "I" in name or k + "_finish" in name for k in kernels):
                    out[g] += ns / 1e6 / CHILD_CALLS
                    launches += count
                    break
        out["launches_per_call"] = launches / CHILD_CALLS
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(profile=True):
    import global_ba_oracle as go
    from morb_slam_amd import Optimizer
    go.lib()              # compiled before any timing
    opt = Optimizer(0)
    for n, reach, points in SIZES:
        p = _problem(n, reach, points)
        kf, mp, st, chi = _call(opt, p)   # warm-up: the workspace grows here
        wall = []
        for _ in range(RUNS):
            t0 = time.perf_counter(); _call(opt, p); wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); want = go.run(p, 10, False); oracle_ms = (time.perf_counter() - t0) * 1e3
        trials = max(int(st[1]), 1)
        res = dict(keyframes=n, reach=reach, points=len(p["mpPos"]), edges=len(p["eKF"]), stats4=st.tolist(), chi2=chi.tolist(),
                   same_path_as_oracle=bool(st.tolist() == want["stats4"].tolist()), worst_pose_difference=float(np.abs(kf - want["kfPose"]).max()),
                   wall_ms=wall, per_trial_ms=[w / trials for w in wall], oracle_ms=oracle_ms, oracle_per_trial_ms=oracle_ms / max(int(want["stats4"][1]), 1))
        split = kernel_split(n, reach, points) if profile else None
        res["kernel_ms_per_call"] = split
        if split:
            res["kernel_ms_per_trial"] = {g: split[g] / trials for g in GROUPS}
            res["factor_us_per_trial_and_block_column"] = split["factor"] / trials / int(st[2]) * 1e3
        print(json.dumps(res), flush=True)
    opt.close()


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main(profile="--no-profile" not in sys.argv)
