#!/usr/bin/env python3
"""Timing of Optimizer::OptimizeEssentialGraph4DoF on MI355X (morb_optimize_essential_graph_4dof) at N = 500 and 2000 keyframes, covisibility
band 10 and 20, one new loop (band + 1 corrected keyframes joined to the loop keyframe: that many long rows) and three old loop edges, 1000
points — the two shapes of tools/bench_essential_graph.py.  In the same process the call alternates with morb_optimize_essential_graph on the
same topology: the same vertices, fixed set and edge list, each measurement the Sim3 of scale 1 that the 4-DoF edge holds, the estimates the
vScw at entry.  Three runs each (host arrays in, host arrays out, warmed up): the wall clock of the synchronous call and the time per LM trial;
beside them the one-thread CPU oracles (tests/native/pose_graph_4dof_oracle.cc, tests/native/essential_graph_oracle.cc), three runs each.
`per_trial_no_slower` is the comparison of the two calls per LM trial with the spread (max - min) of the 7-DoF runs as the margin.
The per-kernel split comes from one more run of the 4-DoF calls in a child process under `rocprofv3 --kernel-trace`: kernel time summed by
name, per call.  --no-profile leaves the split out.  Prints one JSON line per size."""
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
RUNS = 3
CHILD_CALLS = 3
KERNELS = ("k_pg4_linearize", "k_pg4_assemble", "k_pg4_maxdiag", "k_pg4_factor", "k_pg4_backsub", "k_pg4_errors", "k_pg4_decide", "k_pg4_finish")


def _problem(n, band):
    from morb_slam_amd.synth import make_pose_graph_4dof_problem
    return make_pose_graph_4dof_problem(n_kf=n, band=band, n_old_loops=3, n_points=1000, seed=5)


def _sim3_problem(p):
    """The Sim3 pose graph on the 4-DoF problem's topology: EdgeSim3's measurement is Sji, the inverse of the Sij (scale 1) the 4-DoF edge holds."""
    from morb_slam_amd.synth import _quat_from_R_any
    M = np.zeros((len(p["eI"]), 8))
    for e, T in enumerate(p["eTij"]):
        R, t = T[:9].reshape(3, 3), T[9:]
        M[e] = np.concatenate([_quat_from_R_any(R.T), -R.T @ t, [1.0]])
    return dict(kfSim3=p["kfScw"].copy(), kfFlags=(p["kfFixed"] != 0).astype(np.uint8), eI=p["eI"], eJ=p["eJ"], eSji=M, mpPos=p["mpPos"], mpRef=p["mpRef"])


def _call4(opt, p):
    return opt.OptimizeEssentialGraph4DoF(p["kfPose"], p["kfBody"], p["kfFixed"], p["Tcb12"], p["eI"], p["eJ"], p["eTij"], p["mpPos"], p["mpRef"], p["kfScw"])


def _call7(opt, p):
    return opt.OptimizeEssentialGraph(p["kfSim3"], p["kfFlags"], p["eI"], p["eJ"], p["eSji"], p["mpPos"], p["mpRef"])


def child(n, band):
    from morb_slam_amd import Optimizer
    opt, p = Optimizer(0), _problem(n, band)
    for _ in range(CHILD_CALLS):
        _call4(opt, p)
    opt.close()


def kernel_split(n, band):
    """Kernel milliseconds per call by kernel, from a kernel trace of CHILD_CALLS calls; None when the profiler or its database is not there."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    tmp = tempfile.mkdtemp(prefix="bench_pg4_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "-d", tmp, "-o", "pg4", "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(band)],
                           capture_output=True, text=True, timeout=900)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return None
        con = sqlite3.connect(dbs[0])
        rows = con.execute("select s.kernel_name, sum(d.end - d.start), count(*) from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
                           "group by s.kernel_name").fetchall()
        out = {k: 0.0 for k in KERNELS}
        launches = 0
        for name, ns, count in rows:
            for k in KERNELS:
                if k in name:
                    out[k] += ns / 1e6 / CHILD_CALLS
                    launches += count
        out["launches_per_call"] = launches / CHILD_CALLS
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _timed(f, runs=RUNS):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def main(profile=True):
    import essential_graph_oracle as eo
    import pose_graph_4dof_oracle as po
    from morb_slam_amd import Optimizer
    eo.lib(); po.lib()              # compiled before any timing
    opt = Optimizer(0)
    for n, band in SIZES:
        p4 = _problem(n, band)
        p7 = _sim3_problem(p4)
        (P, mp, st4, chi4), (S, _, st7, chi7) = _call4(opt, p4), _call7(opt, p7)   # warm-up: the workspace grows here
        w4, w7 = [], []
        for _ in range(RUNS):       # alternating, in one process and one job
            t0 = time.perf_counter(); _call4(opt, p4); w4.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); _call7(opt, p7); w7.append((time.perf_counter() - t0) * 1e3)
        o4, want4 = _timed(lambda: po.run(p4))
        o7, want7 = _timed(lambda: eo.run(p7))
        t4, t7 = max(int(st4[1]), 1), max(int(st7[1]), 1)
        per4, per7 = [w / t4 for w in w4], [w / t7 for w in w7]
        res = dict(keyframes=n, band=band, edges=len(p4["eI"]), points=len(p4["mpPos"]),
                   dof4=dict(stats4=st4.tolist(), chi2=chi4.tolist(), same_path_as_oracle=bool(st4.tolist() == want4["stats4"].tolist()),
                             worst_pose_difference=float(np.abs(P - want4["kfPose"]).max()), wall_ms=w4, per_trial_ms=per4,
                             per_trial_per_block_column_us=float(np.median(per4)) / int(st4[2]) * 1e3, oracle_ms=o4,
                             oracle_per_trial_ms=[w / max(int(want4["stats4"][1]), 1) for w in o4]),
                   dof7=dict(stats4=st7.tolist(), chi2=chi7.tolist(), same_path_as_oracle=bool(st7.tolist() == want7["stats4"].tolist()),
                             worst_vertex_difference=float(np.abs(S - want7["kfSim3"]).max()), wall_ms=w7, per_trial_ms=per7,
                             per_trial_per_block_column_us=float(np.median(per7)) / int(st7[2]) * 1e3, oracle_ms=o7,
                             oracle_per_trial_ms=[w / max(int(want7["stats4"][1]), 1) for w in o7]))
        res["margin_ms"] = max(per7) - min(per7)
        res["per_trial_no_slower"] = bool(float(np.median(per4)) <= float(np.median(per7)) + res["margin_ms"])
        res["kernel_ms_per_call"] = kernel_split(n, band) if profile else None
        print(json.dumps(res), flush=True)
    opt.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main(profile="--no-profile" not in sys.argv)
