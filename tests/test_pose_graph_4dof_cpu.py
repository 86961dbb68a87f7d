"""Optimizer::OptimizeEssentialGraph4DoF without a GPU: the CPU oracle pinned (error, Jacobian and quadratic form of one free vertex against
numpy central differences of the oracle's own error function; the envelope solve against a dense numpy solve; the gauge of the problem), the
selection of the GPU tests' corpus, the header / export / scratch pins, and the C++ layers as stand-alone programs under sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pose_graph_4dof_cases as cases
import pose_graph_4dof_oracle as po
from morb_slam_amd.synth import make_pose_graph_4dof_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
OMEGA = np.array([1e3, 1e3, 1, 1, 1, 1.0])


def test_oracle_quadratic_form_of_one_free_vertex_against_numpy():
    """A free vertex between two fixed ones, five edges (two of them doubled), the free vertex as vertex 0 of some and vertex 1 of others:
    the oracle's Jacobians, its 4 x 4 H and its b against J^T Omega J and -J^T Omega e, with J from central differences of step 1e-6
    of the oracle's own error function through its own oplus, information weights included.  The oracle's 1e-9 differences carry ~1e-7 of
    relative noise; the bar is 1e-5 of the largest entry (a sign, a transposed block, a missing weight or a missing edge is of order one).
    The free vertex's pose is made the one its body state gives, as after a first accepted update: before it the reference reads the pose as
    given and perturbs the body state, and its error is not the function its Jacobian differentiates."""
    p = make_pose_graph_4dof_problem(n_kf=3, band=2, n_loop=0, seed=40, fixed=(0, 2), meas_noise=0.05, duplicate_every=1)
    assert sorted(zip(p["eI"].tolist(), p["eJ"].tolist())) == [(1, 0), (1, 0), (2, 0), (2, 1), (2, 1)]
    p["kfPose"][1] = po.oplus(p["kfBody"][1], p["Tcb12"], np.zeros(4))
    n, H, b, x, ok, J = po.system(p, 0.0)
    assert n == 1 and H.shape == (4, 4) and ok

    def err(e, u):
        X = p["kfPose"].copy()
        X[1] = po.oplus(p["kfBody"][1], p["Tcb12"], u)
        return po.error(X[p["eI"][e]], X[p["eJ"][e]], p["eTij"][e])

    Hn, bn = np.zeros((4, 4)), np.zeros(4)
    for e in range(len(p["eI"])):
        side = 0 if p["eI"][e] == 1 else 1 if p["eJ"][e] == 1 else None
        if side is None:
            assert not J[e].any()   # an edge between the two fixed vertices has no Jacobian
            continue
        Jn = np.stack([(err(e, 1e-6 * np.eye(4)[k]) - err(e, -1e-6 * np.eye(4)[k])) / 2e-6 for k in range(4)], 1)
        assert np.abs(J[e, side] - Jn).max() <= 1e-5 * np.abs(Jn).max(), e
        assert not J[e, 1 - side].any()
        Hn += Jn.T @ (OMEGA[:, None] * Jn)
        bn -= Jn.T @ (OMEGA * err(e, np.zeros(4)))
    print("H", np.abs(H - Hn).max() / np.abs(Hn).max(), "b", np.abs(b - bn).max() / np.abs(bn).max())
    assert np.abs(Hn).max() > 1 and np.abs(bn).max() > 1e-3
    assert np.abs(H - Hn).max() <= 1e-5 * np.abs(Hn).max() and np.abs(b - bn).max() <= 1e-5 * np.abs(bn).max()
    assert np.abs(H - H.T).max() == 0
    # the error itself: a measurement taken from the two poses gives zero, and a yaw of the first pose shows in the third component only
    Pi, Pj = p["kfPose"][1], p["kfPose"][0]
    Ri, Rj = Pi[:9].reshape(3, 3), Pj[:9].reshape(3, 3)
    T = np.concatenate([(Ri @ Rj.T).ravel(), Pi[9:] - Ri @ Rj.T @ Pj[9:]])
    assert np.abs(po.error(Pi, Pj, T)).max() <= 1e-12


@pytest.mark.parametrize("name", ["n9", "band8", "one_long", "several_fixed"])
def test_oracle_envelope_solve_against_a_dense_solve(name):
    """(H + lambda I) x = b by the oracle's skyline LDL^T against numpy's dense solve of the system it exports, both builds."""
    p = cases.case_problem(name)
    for flags in (po.DEFAULT_FLAGS, po.OTHER_FLAGS):
        n, H, b, x, ok, _ = po.system(p, 0.37, flags)
        assert ok and n == cases.case_oracle(name)["stats4"][2]
        want = np.linalg.solve(H + 0.37 * np.eye(4 * n), b)
        assert np.abs(x - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    assert not po.system(p, -1e12)[4]   # a pivot that is not positive is reported


def test_world_yaw_and_translation_are_gauge():
    """A yaw about the vertical and a translation of the world, applied to every pose, body state and vScw, move the result by the same
    transform to 1e-6: the unknowns are a yaw about the world's vertical and a world translation, and the error is relative.  A roll of the
    world is not gauge: the yaw axis stays the world's z, and the result differs."""
    p = cases.case_problem("n9")
    base = po.run(p)

    def moved(Rw, tw):
        q = dict(p)
        P, B = p["kfPose"].copy(), p["kfBody"].copy()
        for v in range(len(P)):
            Rcw, tcw = p["kfPose"][v, :9].reshape(3, 3), p["kfPose"][v, 9:]
            P[v, :9] = (Rcw @ Rw.T).ravel(); P[v, 9:] = tcw - Rcw @ Rw.T @ tw          # Tcw W^-1
            B[v, :9] = (Rw @ p["kfBody"][v, :9].reshape(3, 3)).ravel(); B[v, 9:] = Rw @ p["kfBody"][v, 9:] + tw   # W Twb
        q["kfPose"], q["kfBody"] = P, B
        q["mpPos"], q["mpRef"] = np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
        r = po.run(q)["kfPose"]
        back = r.copy()
        for v in range(len(r)):
            Rcw, tcw = r[v, :9].reshape(3, 3), r[v, 9:]
            back[v, :9] = (Rcw @ Rw).ravel(); back[v, 9:] = tcw + Rcw @ tw             # (Tcw W^-1) W
        return back

    a = 0.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    d = np.abs(moved(Rz, np.array([3.0, -2.0, 0.5])) - base["kfPose"]).max()
    print("yaw and translation of the world move the result by", d)
    assert d <= 1e-6
    Rx = np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    assert np.abs(moved(Rx, np.zeros(3)) - base["kfPose"]).max() > 1e-4


def test_corpus_selection():
    """Every case through all builds of the oracle (-O2 -ffp-contract=off; -O3 -ffp-contract=fast with the edges summed in reverse; acos / sin
    one ulp off; the matrix a few ulp off before it is factorised): one (iterations, trials) path on every case, no exemption, and poses that
    move by at most 1e-5, a decade under the 1e-4 the GPU is held to.  The chi2 margin of the GPU tests is ten times the largest relative
    spread of the final chi2 between the first two builds.  Then what each class claims is checked on the graph itself."""
    pinned = {n: cases.pinned(n) for n in cases.CASES}
    assert all(pinned.values()), [n for n in pinned if not pinned[n]]
    moved = {n: cases.moved_by_rounding(n) for n in cases.CASES}
    print("poses moved by rounding: at most", max(moved.values()), "at", max(moved, key=moved.get))
    assert max(moved.values()) <= 1e-5
    assert set().union(*(c[0] for c in cases.CASES.values())) == set(cases.CLASSES)
    assert max(len(cases.case_problem(n)["kfPose"]) for n in cases.CASES) <= 200
    spread, where = 0.0, None
    for n in cases.CASES:
        a, b = cases.case_oracle(n), cases.case_oracle(n, po.OTHER_FLAGS)
        assert np.isfinite(a["kfPose"]).all() and a["chi2"][1] <= a["chi2"][0] and a["chi2"][1] > cases.CHI2_FLOOR
        rel = abs(a["chi2"][1] - b["chi2"][1]) / a["chi2"][1]
        if rel > spread:
            spread, where = rel, n
    print("largest relative spread of the final chi2 between the builds:", spread, "at", where, "-> margin", cases.CHI2_MARGIN)
    assert 10 * spread <= cases.CHI2_MARGIN <= 10.5 * spread
    # ---- the classes ----
    rows_per_pass = cases.LINES // 4
    for n, (cl, kw) in cases.CASES.items():
        p, r = cases.case_problem(n), cases.case_oracle(n)
        free = [v for v in range(len(p["kfFixed"])) if not p["kfFixed"][v] and v in set(p["eI"]) | set(p["eJ"])]
        col = {v: i for i, v in enumerate(free)}
        assert r["stats4"][2] == len(free)
        first = list(range(len(free)))
        cyc = len(p["eI"]) - (len(set(p["eI"]) | set(p["eJ"])) - 1)   # edges beyond a spanning tree of a connected graph
        for i, j in zip(p["eI"].tolist(), p["eJ"].tolist()):
            assert i != j
            if i in col and j in col:
                first[max(col[i], col[j])] = min(first[max(col[i], col[j])], col[i], col[j])
        assert r["stats4"][3] == sum(i - f + 1 for i, f in enumerate(first))
        longest = max(i - f for i, f in enumerate(first))
        covering = max(sum(1 for i in range(j, len(free)) if first[i] <= j) for j in range(len(free)))
        long_rows = sum(1 for i, f in enumerate(first) if i - f > kw["band"] + 1)
        if "n2" not in cl: assert cyc >= 1, n   # a cycle (whose measurements do not close: chi2 stays above the floor, above)
        if "stage-1" in cl: assert longest == cases.STAGE - 1, n
        if "stage" in cl: assert longest == cases.STAGE, n
        if "stage+1" in cl: assert longest == cases.STAGE + 1, n
        if not {"stage", "stage+1"} & cl: assert longest < cases.STAGE or "n200" in cl, n
        if "long_span" in cl: assert first[-1] == 0, n
        if "long0" in cl: assert long_rows == 0, n
        if "long1" in cl: assert long_rows == 1, n
        if "long5" in cl: assert long_rows >= 5, n
        if "lines>256" in cl: assert covering > rows_per_pass, n
        else: assert covering <= rows_per_pass, n
        if "n2" in cl: assert len(free) == 1 and len(p["eI"]) == 1 and p["kfFixed"].sum() == 1
        if "n3" in cl: assert len(p["eI"]) == 3 and len(free) == 2
        if "n9" in cl: assert len(p["kfFixed"]) == 9 and len(p["mpPos"]) > 0
        if "n200" in cl: assert len(free) == 199
        if "band1" in cl: assert kw["band"] == 1
        if "band3" in cl: assert kw["band"] == 3
        if "band8" in cl: assert kw["band"] == 8
        if "several_fixed" in cl: assert p["kfFixed"].sum() >= 4
        if "duplicates" in cl: assert len(set(zip(p["eI"].tolist(), p["eJ"].tolist()))) < len(p["eI"])
        if "fixed_pair" in cl: assert any(p["kfFixed"][i] and p["kfFixed"][j] for i, j in zip(p["eI"], p["eJ"]))
        if "isolated" in cl:
            lone = [v for v in kw["isolated"]]
            assert not set(lone) & (set(p["eI"]) | set(p["eJ"])) and r["kfPose"][lone].tobytes() == p["kfPose"][lone].tobytes()
        if "optimum" in cl: assert r["chi2"][1] == r["chi2"][0] and r["stats4"][:2].tolist() == [1, 10] and r["accepted"] == 0 and r["kfPose"].tobytes() == p["kfPose"].tobytes()
        if "stagnation" in cl: assert r["stats4"][:2].tolist() == [3, 3] and r["chi2"][0] > 2e6 and r["chi2"][0] - r["chi2"][1] < 3e-3 * r["chi2"][0]
        if "steps>=5" in cl: assert r["accepted"] >= 5
        if "yaw20" in cl: assert kw["loop_yaw_deg"] == 20 and r["stats4"][0] >= 2 and r["chi2"][0] > 10
        fixed = p["kfFixed"] != 0
        assert r["kfPose"][fixed].tobytes() == p["kfPose"][fixed].tobytes()
        if len(p["mpPos"]):
            skip = p["mpRef"] < 0
            assert (skip.any() or len(skip) < 10) and r["mpPos"][skip].tobytes() == p["mpPos"][skip].tobytes(), n
            if "optimum" not in cl:
                assert np.isfinite(r["mpPos"]).all() and np.abs(r["mpPos"][~skip] - p["mpPos"][~skip]).max() > 1e-4, n


def test_header_declares_and_library_exports_the_entry():
    from morb_slam_amd.capi import HEADER
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_optimize_essential_graph_4dof\(morb_optimizer\*, int nKF, double\* kfPose, const double\* kfBody, const uint8_t\* kfFixed,", header)
    assert "morb_optimize_essential_graph_4dof" in HEADER.prototypes and len(HEADER.prototypes["morb_optimize_essential_graph_4dof"][1]) == 16
    assert "Optimizer.cc:5163-5472" in header and ":5451-5470" in header
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    assert hasattr(ctypes.CDLL(LIB), "morb_optimize_essential_graph_4dof")


SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPG4_STUB_ENTRY", "-D__HIP_PLATFORM_AMD__"]


def test_view_adapter_under_sanitizers(tmp_path):
    """tests/native/pose_graph_4dof_adapter_check.cc with the C entry stubbed to record its arguments, built as a stand-alone program with
    -fsanitize=address,undefined: Optimizer::OptimizeEssentialGraph4DoF(PoseGraph4DoFView&) hands the entry the view's arrays unchanged and in
    the entry's order, with and without points, and the view holds the entry's results afterwards."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "pose_graph_4dof_adapter_check")
    subprocess.check_call(SAN + ["-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                                 os.path.join(native, "pose_graph_4dof_adapter_check.cc")])
    for name in ("n9", "duplicates"):
        p = dict(cases.case_problem(name))
        if name == "duplicates":
            p["mpPos"], p["mpRef"] = np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        given = cases.problem_bytes(p)
        open(fin, "wb").write(given)
        out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "pose graph 4dof view ok" in out.stdout, out.stdout + out.stderr
        raw = open(fout, "rb").read()
        nKF, nMP = len(p["kfPose"]), len(p["mpPos"])
        recorded = given if nMP else given[:len(given) - 64 * nKF]   # (vScw is not read without points)
        assert raw[:len(recorded)] == recorded
        want = (100.0 + np.arange(12 * nKF)).tobytes() + (200 + np.arange(3 * nMP)).astype(np.float32).tobytes() + np.array([3, 12, nKF - 1, 77], np.int32).tobytes() + \
            np.array([5.5, 0.25]).tobytes()
        assert raw[len(recorded):] == want


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/pose_graph_4dof_member_check.cc: the call expression of LoopClosing.cc:1201-1203 unedited on a mock map of seven keyframes,
    with the C entry stubbed in the program to compare the flattened graph with an expectation written out by hand — vertices in ascending mnId
    without the bad keyframe, the loop keyframe fixed, the 12 edges of Optimizer.cc:5236-5426 in insertion order (a weight below 100 on and off
    the (cur, loop) pair, a pair already in sInsertedEdges, mPrevKF / mNextKF / child / loop-edge / bad / later covisibles, an old loop edge, an
    mPrevKF link to a bad keyframe), each Tij from the corrected or the non-corrected Sim3 as the reference takes it, a corrected keyframe of
    scale 1.03 built from the inverse of its Sim3, the points' references — and then the write-back: SetPose, SetWorldPos,
    UpdateNormalAndDepth, IncreaseChangeIndex.  Built with -fsanitize=address,undefined as a stand-alone program."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "pose_graph_4dof_member_check")
    subprocess.check_call(SAN + ["-I" + os.path.join(native, "mock_pose_graph_4dof"), "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"),
                                 "-I/opt/rocm/include", "-o", exe, os.path.join(native, "pose_graph_4dof_member_check.cc")])
    src = open(os.path.join(native, "pose_graph_4dof_member_check.cc")).read()
    assert ("Optimizer::OptimizeEssentialGraph4DoF(pLoopMap, mpLoopMatchedKF,\n                                          mpCurrentKF, NonCorrectedSim3,\n"
            "                                          CorrectedSim3, LoopConnections);") in src
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pose graph 4dof member ok" in out.stdout, out.stdout + out.stderr


def test_kernel_scratch_is_pinned(tmp_path):
    """None of the eight kernels uses scratch memory: no array of theirs is indexed by a run-time value, the perturbed states of the numeric
    Jacobians stay in registers, and the factorisation's column loop touches registers, LDS and the envelope only."""
    import test_codeobj_cpu as co
    if not (os.path.exists(LIB) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(LIB, str(tmp_path)).items() if "k_pg4_" in k}
    short = {re.search(r"\d+(k_pg4_[a-z]+)E", k).group(1): v for k, v in meta.items()}
    assert short == {"k_pg4_linearize": 0, "k_pg4_assemble": 0, "k_pg4_maxdiag": 0, "k_pg4_factor": 0, "k_pg4_backsub": 0, "k_pg4_errors": 0, "k_pg4_decide": 0,
                     "k_pg4_finish": 0}, short
    for pats in (co.HOT, co.BOUNDED):   # the names stay clear of the lists of tests/test_codeobj_cpu.py
        assert not any(re.search(r"\d+" + s + r"(I|E)", k) for s in pats for k in meta)
    assert not any("k_eg_" in k for k in meta)
