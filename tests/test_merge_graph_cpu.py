"""The second overload of Optimizer::OptimizeEssentialGraph (map merging) without a GPU: the CPU oracle's preparation pinned on a
hand-written graph, the selection of the GPU tests' corpus, the header / export pins, the call site of LoopClosing::MergeLocal against
mocks, and the reference-typed member's flattening and write-back on a mock map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import merge_graph_cases as cases
import merge_graph_oracle as mo
from morb_slam_amd.synth import _quat_from_rotvec, _sim3_inv, _sim3_mul, make_merge_graph_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
NATIVE = os.path.join(ROOT, "tests", "native")


def _pose(rotvec, t):
    return np.concatenate([_quat_from_rotvec(np.array(rotvec, np.float64)), t]).astype(np.float32)


def _sim3(p):
    """g2o::Sim3 of a float pose: the quaternion normalised in FP64, s = 1."""
    p = p.astype(np.float64)
    return np.concatenate([p[:4] / np.linalg.norm(p[:4]), p[4:7], [1.0]])


def _same(a, b, tol=1e-12):
    b = b.copy()
    if np.dot(a[:4], b[:4]) < 0:
        b[:4] = -b[:4]
    return np.abs(a - b).max() <= tol


def test_kept_edges_and_measurements_of_a_hand_written_graph():
    """Six keyframes: v0, v1 in vpFixedKFs, v2 in vpFixedCorrectedKFs alone, v3 in the window and the non-fixed list, v4, v5 non-fixed.  Nine
    candidates, their measurements written out below from the reference's rules (Optimizer.cc:1892-1916) with numpy's Sim3 algebra: the
    identity Swi of a vpFixedKFs keyframe (the measurement is the other end's pose itself), the mixed measurement of a window keyframe
    against a good one (the other end's corrected pose times the inverse of its own pose before the merge), vScw on both sides of a bad
    pair, and the three good / bad pairs that have no edge.  Estimates: the pose, never mTcwBefMerge; fixed and _fix_scale as the lists say."""
    Tcw = np.stack([_pose([0.1 * k, -0.2 + 0.05 * k, 0.03 * k], [1.0 + 0.7 * k, -0.3 * k, 2.0 - 0.4 * k]) for k in range(6)])
    Bef = np.stack([_pose([0.1 * k + 0.04, -0.25 + 0.05 * k, 0.02 * k], [1.5 + 0.7 * k, -0.3 * k + 0.2, 2.3 - 0.4 * k]) for k in range(6)])
    lists = np.array([1, 1, 2, 6, 4, 4], np.uint8)
    cand = [(1, 0), (1, 2), (2, 1), (3, 2), (4, 3), (5, 4), (4, 1), (0, 4), (5, 0)]
    S, B = [_sim3(p) for p in Tcw], [_sim3(p) for p in Bef]
    want = {
        (1, 0): S[0],                               # good pair, i in vpFixedKFs: Swi is g2o::Sim3(), the measurement is Sjw
        (1, 2): S[2],                               # ... also against a window keyframe: its corrected pose
        (2, 1): _sim3_mul(S[1], _sim3_inv(B[2])),   # good pair, i in the window: j's corrected pose, i's pose before the merge
        (3, 2): _sim3_mul(S[2], _sim3_inv(B[3])),   # both in the window: good wins, the same mix
        (4, 3): _sim3_mul(B[3], _sim3_inv(S[4])),   # bad pair: vScw[j] = mTcwBefMerge of the window keyframe, vScw[i] = the pose
        (5, 4): _sim3_mul(S[4], _sim3_inv(S[5])),   # two non-fixed keyframes
    }
    prob = dict(kfLists=lists, kfTcw=Tcw, kfTwc=Tcw, kfTcwBefMerge=Bef, kfTwcBefMerge=Bef, cI=[c[0] for c in cand], cJ=[c[1] for c in cand])
    for flags in (mo.DEFAULT_FLAGS, mo.OTHER_FLAGS):
        g = mo.prepare(prob, flags)
        assert g["cKept"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0]
        assert list(zip(g["eI"].tolist(), g["eJ"].tolist())) == cand[:6]
        for e, c in enumerate(cand[:6]):
            assert _same(want[c], g["eSji"][e]), (c, want[c], g["eSji"][e])
        assert g["kfFlags"].tolist() == [3, 3, 1, 1, 0, 0]
        for v in range(6):
            assert _same(S[v], g["kfSim3"][v], 1e-15) and g["kfSim3"][v, 7] == 1.0 and abs(np.linalg.norm(g["kfSim3"][v, :4]) - 1) < 4e-16
    assert not _same(want[(2, 1)], _sim3_mul(S[1], _sim3_inv(S[2])), 1e-3)   # (what a "fixed" measurement would be)


def test_corpus_selection():
    """Every case through the two builds of the oracle and the four perturbed ones (essential_graph_oracle.py).  Only cases on whose
    (iterations, trials) the two builds agree pin the GPU's path: at least half of the cases and at least one of every class, and each of
    them holds under the perturbed builds too, none of which moves a pose or a point by more than a third of the 1e-4 the GPU is held to.
    The chi2 margin of the GPU tests is ten times the largest relative spread of the final chi2 between the two builds over those cases.
    Then what each class claims is checked on the problem itself."""
    agree = {n: cases.builds_agree(n) for n in cases.CASES}
    print("LM path agrees on", sum(agree.values()), "of", len(agree), "cases; differs on", [n for n in agree if not agree[n]])
    assert 2 * sum(agree.values()) >= len(agree)
    for k in cases.CLASSES:
        assert any(agree[n] for n in cases.CASES if k in cases.CASES[n][0]), k
    pinned = {n: cases.pinned(n) for n in cases.CASES}
    assert all(pinned[n] for n in cases.CASES if agree[n]), [n for n in cases.CASES if agree[n] and not pinned[n]]
    moved = {n: cases.moved_by_rounding(n) for n in cases.CASES}
    print("poses and points moved by rounding: at most", max(moved.values()), "at", max(moved, key=moved.get))
    assert max(moved.values()) <= 1e-4 / 3
    assert set().union(*(c[0] for c in cases.CASES.values())) == set(cases.CLASSES)
    spread, where = 0.0, None
    for n in cases.CASES:
        a, b = cases.case_oracle(n), cases.case_oracle(n, mo.OTHER_FLAGS)
        assert all(np.isfinite(a[k]).all() for k in mo.POSES) and a["chi2"][1] <= a["chi2"][0]
        if agree[n] and a["chi2"][1] > cases.CHI2_FLOOR:
            rel = abs(a["chi2"][1] - b["chi2"][1]) / a["chi2"][1]
            if rel > spread:
                spread, where = rel, n
    print("largest relative spread of the final chi2 between the builds:", spread, "at", where, "-> margin", cases.CHI2_MARGIN)
    assert 10 * spread <= cases.CHI2_MARGIN <= 10.5 * spread
    # ---- the classes ----
    for n, (cl, kw) in cases.CASES.items():
        p, r = cases.case_problem(n), cases.case_oracle(n)
        lists, cI, cJ = p["kfLists"], p["cI"], p["cJ"]
        assert set(lists.tolist()) <= {1, 2, 4, 6} and (cI != cJ).all()
        good, bad = (lists & 3) != 0, (lists & 6) != 0
        kept = (good[cI] & good[cJ]) | (bad[cI] & bad[cJ])
        assert r["cKept"].tolist() == kept.astype(np.uint8).tolist()
        with_edge = np.isin(np.arange(len(lists)), np.concatenate([cI[kept], cJ[kept]]))
        free = (lists == 4) & with_edge
        assert r["stats4"][2] == free.sum()
        tail = (lists & 4) != 0
        for k, src in (("kfTcwBefMerge", "kfTcw"), ("kfTwcBefMerge", "kfTwc")):   # the BefMerge members: the entry pose behind the tail, untouched elsewhere
            assert r[k][tail].tobytes() == p[src][tail].tobytes() and r[k][~tail].tobytes() == p[k][~tail].tobytes()
        for k in ("kfTcw", "kfTwc"):
            assert r[k][~tail].tobytes() == p[k][~tail].tobytes()
            still = tail & ~free   # fixed-corrected keyframes of the non-fixed list, free ones without an edge: a float -> double -> float round trip
            assert np.abs(cases.pose_diff(r[k][still], p[k][still])).max(initial=0) <= 1e-6 * max(1.0, np.abs(p[k]).max())
        fixed_fixed = kept & (lists[cI] != 4) & (lists[cJ] != 4)
        if "smallest" in cl: assert lists.tolist() == [1, 4, 2] and free.sum() == 1 and kept.sum() == 2
        if "merge" in cl: assert ((lists == 1).sum(), (lists & 2 != 0).sum(), (lists & 4 != 0).sum()) == (6, 5, 20) and fixed_fixed.sum() > 10
        if "stagnation" in cl:   # three accepted iterations, each gaining less than a thousandth of chi2, and still a solve that moves the map
            assert r["stats4"][:2].tolist() == [3, 3] and 0 < r["chi2"][0] - r["chi2"][1] < 1e-3 * r["chi2"][1]
            assert np.abs(r["kfTcw"][free] - p["kfTcw"][free]).max() > 0.1
        if "no_fixed_edge" in cl: assert not fixed_fixed.any() and r["stats4"][0] > 3
        else: assert fixed_fixed.any() or n == "no_fixed_edge_b"
        if "panel+1" in cl: assert free.sum() > cases.PANEL + 1 and r["stats4"][3] >= free.sum() + cases.PANEL + 1
        if "inside" in cl: assert ((lists & 2) != 0).any() and (lists[(lists & 2) != 0] == 6).all()
        if "disjoint" in cl: assert (lists == 2).any() and not (lists == 6).any()
        if "bad_parent" in cl:   # against the same map with every keyframe alive: the child's spanning-tree candidate is gone and nothing stands in for it
            ids = p["ids"]
            q = make_merge_graph_problem(**{**kw, "bad": ()})
            for b in kw["bad"]:
                child = int(np.searchsorted(ids, b))
                assert b not in ids and ids[child] == b + 1
                alive = [int(j) for j in q["cJ"][q["cI"] == b + 1]]
                assert alive[0] == b and [int(ids[j]) for j in cJ[cI == child]] == [j for j in alive if j not in kw["bad"]]
        if "no_edge" in cl:
            lone = [int(np.searchsorted(p["ids"], i)) for i in kw["isolated"]]
            assert not with_edge[lone].any() and (lists[lone] == 4).all() and all((cI == v).sum() == 1 for v in lone) and not kept[np.isin(cI, lone)].any()
        if "no_free" in cl: assert free.sum() == 0 and r["stats4"].tolist() == [0, 0, 0, 0] and r["chi2"].tolist() == [0.0, 0.0] and tail.any() and kept.any()
        else: assert free.sum() > 0 and r["stats4"][0] > 0 and r["chi2"][1] < r["chi2"][0]
        ref = p["mpRef"]
        if "points_each_list" in cl:
            assert all((lists[ref[ref >= 0]] == l).any() for l in set(lists.tolist())) and (ref < 0).any()
        if "no_points" in cl: assert len(ref) == 0
        if len(ref):
            stays = (ref < 0) | (lists[np.maximum(ref, 0)] == 1)
            assert r["mpPos"][stays].tobytes() == p["mpPos"][stays].tobytes()
            through_moved = ~stays & np.isin(ref, np.flatnonzero(free))
            if through_moved.any():
                assert np.abs(r["mpPos"][through_moved] - p["mpPos"][through_moved]).max() > 1e-3
            assert np.isfinite(r["mpPos"]).all()


def test_header_declares_and_library_exports_the_entry():
    from morb_slam_amd.capi import HEADER
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_optimize_essential_graph_merge\(morb_optimizer\*, int nKF, const uint8_t\* kfLists, float\* kfTcw, float\* kfTwc,", header)
    assert "morb_optimize_essential_graph_merge" in HEADER.prototypes and len(HEADER.prototypes["morb_optimize_essential_graph_merge"][1]) == 16
    assert "Optimizer.cc:1737-2063" in header and "LoopClosing.cc:1747-1749" in header
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    assert hasattr(ctypes.CDLL(LIB), "morb_optimize_essential_graph_merge")


def _includes():
    return ["-I" + os.path.join(NATIVE, "mock_merge_graph"), "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]


def test_call_site_of_merge_local_compiles_unchanged(tmp_path):
    """tests/native/merge_graph_call_check.cc holds the call expression of LoopClosing.cc:1747-1749 verbatim; against the mocks of
    tests/native/mock_merge_graph it picks the member template of overload 2 and instantiates it."""
    src = open(os.path.join(NATIVE, "merge_graph_call_check.cc")).read()
    assert ("      Optimizer::OptimizeEssentialGraph(mpCurrentKF, vpMergeConnectedKFs,\n                                        vpLocalCurrentWindowKFs,\n"
            "                                        vpCurrentMapKFs, vpCurrentMapMPs);") in src
    obj = str(tmp_path / "merge_graph_call_check.o")
    subprocess.check_call(["g++", "-std=c++17", "-c", "-D__HIP_PLATFORM_AMD__", *_includes(), "-o", obj, os.path.join(NATIVE, "merge_graph_call_check.cc")])
    syms = subprocess.run(["nm", "-C", obj], capture_output=True, text=True, check=True).stdout
    assert re.search(r"W void ORB_SLAM3::Optimizer::OptimizeEssentialGraph<ORB_SLAM3::MGKeyFrame, ORB_SLAM3::MGMapPoint>\(", syms), syms
    assert "flatten_merge_graph<ORB_SLAM3::MGKeyFrame, ORB_SLAM3::MGMapPoint>" in syms


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/merge_graph_member_check.cc: the same call expression on a mock map of ten keyframes, with the C entry stubbed in the
    program to compare the flattened problem with an expectation written out by hand — vertices in ascending mnId without the bad keyframe,
    their lists, the four poses of each, the 19 candidates of Optimizer.cc:1888-1999 in insertion order with the window's keyframes visited
    twice, the points' references behind the EraseObservation loop — and then the write-back: mTcwBefMerge, mTwcBefMerge and SetPose on
    the non-bad keyframes of vpNonFixedKFs only, SetWorldPos and UpdateNormalAndDepth on the points whose reference is bad-flagged.  Built with
    -fsanitize=address,undefined as a stand-alone program."""
    exe = str(tmp_path / "merge_graph_member_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMG_STUB_ENTRY", "-D__HIP_PLATFORM_AMD__",
                           *_includes(), "-o", exe, os.path.join(NATIVE, "merge_graph_member_check.cc")])
    src = open(os.path.join(NATIVE, "merge_graph_member_check.cc")).read()
    assert src.count("      Optimizer::OptimizeEssentialGraph(mpCurrentKF, vpMergeConnectedKFs,\n                                        vpLocalCurrentWindowKFs,\n"
                     "                                        vpCurrentMapKFs, vpCurrentMapMPs);") == 2
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "merge graph member ok" in out.stdout, out.stdout + out.stderr
