#!/usr/bin/env python3
"""Timing of Optimizer::OptimizeEssentialGraph on MI355X (morb_optimize_essential_graph) at N = 500 and 2000 keyframes, covisibility band 10
and 20, one new loop (band + 1 corrected keyframes joined to the loop keyframe: that many long rows) and three old loop edges, 1000 points.
Per call (host arrays in, host arrays out, warmed up): the wall clock of the synchronous call; beside it the one-thread CPU oracle
(tests/native/essential_graph_oracle.cc) on the same problem, the LM work covered (iterations, trials) and the size of the system.
The phase split comes from a second run of the same calls in a child process under `rocprofv3 --kernel-trace`: kernel time summed by
name into edges (k_eg_linearize, k_eg_assemble), factorisation (k_eg_factor, with the forward substitution that rides on it), substitution
(k_eg_backsub, with the trial estimates) and trial chi2 (k_eg_errors, k_eg_decide), per call.  --no-profile leaves the split out.
Prints one JSON line per size; numbers only, no threshold."""
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

SIZES = ((500, 10), (2000, 20))
CHILD_CALLS = 3
PHASES = {"k_eg_linearize": "edges", "k_eg_assemble": "edges", "k_eg_factor": "factorisation", "k_eg_backsub": "substitution",
          "k_eg_errors": "trial_chi2", "k_eg_decide": "trial_chi2", "k_eg_finish": "points"}


def _problem(n, band):
    from morb_slam_amd.synth import make_essential_graph_problem
    return make_essential_graph_problem(n_kf=n, band=band, n_old_loops=3, n_points=1000, seed=5)


def _call(opt, p):
    return opt.OptimizeEssentialGraph(p["kfSim3"], p["kfFlags"], p["eI"], p["eJ"], p["eSji"], p["mpPos"], p["mpRef"])


def child(n, band):
    from morb_slam_amd import Optimizer
    opt, p = Optimizer(0), _problem(n, band)
    for _ in range(CHILD_CALLS):
        _call(opt, p)
    opt.close()


def phase_split(n, band):
    """Kernel milliseconds per call by phase, from a kernel trace of CHILD_CALLS calls; None when the profiler or its database is not there."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    tmp = tempfile.mkdtemp(prefix="bench_eg_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "-d", tmp, "-o", "eg", "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(band)],
                           capture_output=True, text=True, timeout=900)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return None
        con = sqlite3.connect(dbs[0])
        rows = con.execute("select s.kernel_name, sum(d.end - d.start), count(*) from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
                           "group by s.kernel_name").fetchall()
        out = {v: 0.0 for v in PHASES.values()}
        launches = 0
        for name, ns, count in rows:
            for k, phase in PHASES.items():
                if k in name:
                    out[phase] += ns / 1e6 / CHILD_CALLS
                    launches += count
        out["launches_per_call"] = launches / CHILD_CALLS
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(reps=5, profile=True):
    import essential_graph_oracle as eo
    from morb_slam_amd import Optimizer
    eo.lib()                        # compiled before any timing
    opt = Optimizer(0)
    for n, band in SIZES:
        p = _problem(n, band)
        S, mp, stats, chi2 = _call(opt, p)
        t0 = time.perf_counter()
        want = eo.run(p)
        oracle_ms = (time.perf_counter() - t0) * 1e3
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _call(opt, p)
            wall.append((time.perf_counter() - t0) * 1e3)
        res = dict(keyframes=n, band=band, edges=len(p["eI"]), points=len(p["mpPos"]), stats4=stats.tolist(), chi2=chi2.tolist(),
                   same_path_as_oracle=bool(stats.tolist() == want["stats4"].tolist()), worst_vertex_difference=float(np.abs(S - want["kfSim3"]).max()),
                   oracle_ms=oracle_ms, wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                   per_trial_ms=float(np.median(wall)) / max(int(stats[1]), 1), per_trial_per_block_column_us=float(np.median(wall)) / max(int(stats[1]), 1) / int(stats[2]) * 1e3)
        res["kernel_ms_per_call_by_phase"] = phase_split(n, band) if profile else None
        print(json.dumps(res), flush=True)
    opt.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main(profile="--no-profile" not in sys.argv)
