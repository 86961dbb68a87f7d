"""The whole-map bundle adjustment of loop closing without a GPU: the skyline oracle pinned to the dense welding-BA oracle already in the tree,
the selection of the GPU tests' corpus and what its scenes exercise, the header / export pins and the kernels' scratch memory."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import global_ba_cases as cases
import global_ba_oracle as go
import merge_ba_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINHOLE = [c for c in cases.CASES if c[0] != "kb8"]


@pytest.mark.parametrize("case", PINHOLE, ids=cases.case_id)
def test_oracle_is_the_dense_oracle_on_pinhole_cases(case):
    """tests/native/merge_ba_oracle.cc as one round of n iterations with delta^2 5.99 is this function on a pinhole map: an independent
    restatement with a dense reduced system and a dense LDL^T.  Same (iterations, trials); poses and points within 1e-9."""
    p, a = cases.scene(case), cases.case_oracle(case)
    m = mo.run(p, plan=((case[6], case[5], 5.99),))
    assert a["stats4"][:2].tolist() == m["stats6"][:2].tolist()
    assert np.abs(a["kfPose"].astype(np.float64) - m["kfPose"]).max() <= 1e-9 and np.abs(a["mpPos"].astype(np.float64) - m["mpPos"]).max() <= 1e-9


def _differ(a, b):
    if a["stats4"].tolist() != b["stats4"].tolist():
        return True
    return max(np.abs(a["kfPose"].astype(np.float64) - b["kfPose"]).max(), np.abs(a["mpPos"].astype(np.float64) - b["mpPos"]).max()) > 1e-6


def test_corpus_selection():
    """Every case of the GPU corpus through two builds of the oracle (-O2 -ffp-contract=off, points in order; -O3 -ffp-contract=fast, points in
    reverse): a case whose stats differ, or whose outputs differ by more than 1e-6, turns on the rounding of a sum and is no test of a kernel;
    it is listed in cases.LEFT_OUT — at most one in ten.  Prints the largest relative chi2 spread between the builds over the kept cases: ten
    times that is the GPU tests' chi2 bound (CHI2_SPREAD in tests/global_ba_cases.py)."""
    differ = [c for c in cases.CASES if _differ(cases.case_oracle(c), cases.case_oracle(c, go.OTHER_FLAGS))]
    print("cases that differ between the two builds:", differ)
    assert set(differ) <= cases.LEFT_OUT, differ
    assert cases.LEFT_OUT <= set(cases.CASES) and len(cases.LEFT_OUT) * 10 <= len(cases.CASES)
    spread = 0.0
    for c in cases.CASES:
        if c not in cases.LEFT_OUT:
            a, b = cases.case_oracle(c)["chi2"], cases.case_oracle(c, go.OTHER_FLAGS)["chi2"]
            spread = max(spread, float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
    print("largest relative chi2 spread between the two builds:", spread)
    assert spread <= cases.CHI2_SPREAD


X87_FLAGS = ("-O2", "-ffp-contract=off", "-mfpmath=387")   # a third rounding convention: sums and products kept in extended precision


def test_kb8_cases_do_not_turn_on_a_step_of_the_float_projection():
    """KannalaBrandt8::project's atan2f makes chi2 a staircase in the estimate (tests/global_ba_cases.py, _RESEED): a KannalaBrandt8 case is
    kept only with a seed on which a third build of the oracle, with x87 arithmetic, follows the first one within the spread the chi2 bound
    is derived from.  (The pinhole cases have no such step; FACTOR_FAILS lives on the doubles' exponent range, which x87 registers exceed.)"""
    try:
        go.lib(X87_FLAGS)
    except subprocess.CalledProcessError:
        return   # (not an x86 host: the seeds were chosen where this build exists)
    for c in cases.CASES:
        if c[0] == "kb8" and c not in cases.LEFT_OUT:
            a, b = cases.case_oracle(c), cases.case_oracle(c, X87_FLAGS)
            assert a["stats4"].tolist() == b["stats4"].tolist(), c
            assert (np.abs(a["chi2"] - b["chi2"]) <= cases.CHI2_SPREAD * np.maximum(1.0, np.abs(a["chi2"]))).all(), c


def test_corpus_covers_the_grid():
    kept = [c for c in cases.CASES if c not in cases.LEFT_OUT]
    assert {(c[0], c[5], c[1] - 1) for c in kept if c in cases.SMALL} == {(cam, r, f) for cam in cases.CAMS for r in (0, 1) for f in (1, 2, 3)}
    for c in kept:
        p = cases.scene(c)
        assert len(p["kfPose"]) <= 125 and len(p["mpPos"]) <= 2100 and len(p["eKF"]) <= 15000
        if c[0] == "mix":
            assert (p["eObs"][:, 2] < 0).any() and (p["eObs"][:, 2] >= 0).any()
        if c[0] == "mono":
            assert (p["eObs"][:, 2] < 0).all()
        if c[0] == "kb8":   # right-camera edges, each behind the left edge of the same (keyframe, point) pair
            r = np.flatnonzero(p["rig"]["eRight"])
            assert len(r) and (p["eKF"][r] == p["eKF"][r - 1]).all() and (p["eMP"][r] == p["eMP"][r - 1]).all() and not p["rig"]["eRight"][r - 1].any()
    for c in cases.SMALL:
        col, first, count = cases.structure(cases.scene(c))
        assert (col >= 0).sum() == c[1] - 1
    for cam in cases.CAMS:   # reach 1 without loop points: a block-tridiagonal system; reach 30: full; loop points: long rows at the end
        by = {(c[2], c[4]): cases.structure(cases.scene(c)) for c in cases.SHAPES if c[0] == cam}
        col, first, count = by[(1, 0)]
        assert (np.arange(len(first)) - first).max() == 1
        col, first, count = by[(30, 0)]
        assert not first.any() and len(count) == len(first) * (len(first) + 1) // 2
        col, first, count = by[(1, 6)]
        assert first[-1] == 0 and (np.arange(len(first)) - first)[3:-3].max() == 1
        col, first, count = by[(6, 6)]
        assert first[-1] == 0 and (np.arange(len(first)) - first)[3:-3].max() == 6


def test_tier_edge_scenes_sit_on_the_constants():
    """One below, on and one above each tier constant of csrc/global_ba.hip, read off the scenes' own edge lists."""
    src = open(os.path.join(ROOT, "morb_slam_amd", "csrc", "global_ba.hip")).read()
    assert re.search(r"GBA_NT = 256;", src) and re.search(r"GBA_ROWS = GBA_NT / 6;", src) and cases.ROWS_PER_PASS == 256 // 6
    assert re.search(r"GBA_STAGE = %d;" % cases.LDS_PANEL, src) and re.search(r"GBA_CHUNK = %d;" % cases.CHUNK, src)
    got = []
    for c in cases.ROWS_EDGE:   # rows covering column 0, the diagonal block's among them
        col, first, count = cases.structure(cases.scene(c))
        got.append(int((first == 0).sum()))
    assert got == [cases.ROWS_PER_PASS - 1, cases.ROWS_PER_PASS, cases.ROWS_PER_PASS + 1]
    got = []
    for c in cases.PANEL_EDGE:   # blocks of the last row in front of its diagonal block
        col, first, count = cases.structure(cases.scene(c))
        got.append(int(len(first) - 1 - first[-1]))
    assert got == [cases.LDS_PANEL - 1, cases.LDS_PANEL, cases.LDS_PANEL + 1]
    got = []
    for c in cases.CHUNK_EDGE:
        col, first, count = cases.structure(cases.scene(c))
        assert set(count) == {(0, 0), (1, 0), (1, 1)} and len(set(count.values())) == 1
        got.append(count[(1, 0)])
    assert got == [cases.CHUNK - 1, cases.CHUNK, cases.CHUNK + 1] * 2


def test_named_scenes_do_what_their_names_say():
    for c in cases.NAMED:
        assert c not in cases.LEFT_OUT
    for c in (cases.SPARSE_POINTS, cases.SPARSE_POINTS_KB8):
        p = cases.scene(c)
        free = p["kfFixed"] == 0
        per_point = [p["eKF"][p["eMP"] == m] for m in range(len(p["mpPos"]))]
        assert sum(1 for k in per_point if len(set(k.tolist())) == 1 and free[k[0]]) >= 6      # one free keyframe only: no pair
        assert sum(1 for k in per_point if len(k) and not free[k].any()) == 3                  # fixed keyframes only
        assert len(p["mono_single"]) == 3
        for m in p["mono_single"]:                                                           # one monocular observation
            e = np.flatnonzero(p["eMP"] == m)
            assert len(e) == 1 and (p["rig"] is not None or p["eObs"][e[0], 2] < 0)
    p, r = cases.scene(cases.IDLE), cases.case_oracle(cases.IDLE)
    assert not p["kfFixed"][5] and not (p["eKF"] == 5).any()
    idle = np.setdiff1d(np.arange(len(p["mpPos"])), p["eMP"])
    assert len(idle) == 2
    assert r["kfPose"][5].tobytes() == p["kfPose"][5].tobytes() and r["mpPos"][idle].tobytes() == p["mpPos"][idle].tobytes()
    assert r["stats4"][2] == len(p["kfPose"]) - 2
    p = cases.scene(cases.TWO_FIXED)
    assert p["kfFixed"].tolist()[:3] == [1, 1, 0] and p["kfFixed"].sum() == 2
    assert cases.case_oracle(cases.ONE_ITERATION)["stats4"][:2].tolist() == [1, 1]
    p, r = cases.scene(cases.AT_TRUTH), cases.case_oracle(cases.AT_TRUTH)
    assert np.abs(p["kfPose"] - p["true_poses"]).max() < 1e-6 and r["chi2"][0] < 1e-6
    assert r["stats4"][1] > r["stats4"][0] and r["stats4"][0] < 10                            # rejected trials, and they end the optimisation
    for c in (cases.FACTOR_FAILS, cases.FACTOR_FAILS_ROBUST):                               # ten failed factorisations, nothing moves
        p, r = cases.scene(c), cases.case_oracle(c)
        assert r["stats4"][:2].tolist() == [1, 10] and np.isfinite(r["chi2"]).all() and r["chi2"][0] == r["chi2"][1]
        assert r["kfPose"].tobytes() == p["kfPose"].tobytes() and r["mpPos"].tobytes() == p["mpPos"].tobytes()


def test_stop_at_entry_of_the_oracle():
    p = cases.scene(cases.SMALL[2])
    r = go.run(p, stop_entry=True)
    assert r["stats4"].tolist() == [0] * 4 and r["kfPose"].tobytes() == p["kfPose"].tobytes() and r["mpPos"].tobytes() == p["mpPos"].tobytes()


def test_header_declares_and_library_exports_the_entries():
    from morb_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_bundle_adjustment\(morb_optimizer\*, int nKF, float\* kfPose, const uint8_t\* kfFixed, int nMP, float\* mpPos,", header)
    assert "Optimizer.cc:56-362" in header and "LoopClosing.cc:2302" in header
    for name, nargs in (("morb_bundle_adjustment", 21), ("morb_bundle_adjustment_fisheye", 20)):
        restype, argtypes = capi.HEADER.prototypes[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    assert capi.HEADER.prototypes["morb_bundle_adjustment"][1][11:16] == [ctypes.c_float] * 5
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("library not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.lib()
    for name in ("morb_bundle_adjustment", "morb_bundle_adjustment_fisheye"):
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert list(getattr(L, name).argtypes) == capi.HEADER.prototypes[name][1]     # the parsed prototype went through capi.py's loop


def test_kernels_use_no_scratch_memory(tmp_path):
    import test_codeobj_cpu as co
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    if not (os.path.exists(lib) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(lib, str(tmp_path)).items() if re.search(r"\d+k_gba_\w+?(I|E)", k)}
    assert len(meta) == 12, meta          # eleven kernels, k_gba_linearize in its pinhole and KannalaBrandt8 forms
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/global_ba_member_check.cc: the host-only flattening of WholeMapBundleAdjustment against an edge list written by hand (a bad
    keyframe, a bad point, a keyframe outside vpKFs, a point without an edge, a rig keyframe with left and right observations), the write-back
    for both nLoopKF cases, and GlobalBundleAdjustemnt with LoopClosing's five arguments under MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT, with the C
    entries stubbed in the program; built with -fsanitize=address,undefined as a stand-alone program."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "global_ba_member_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(native, "mock_global_ba"), "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-o", exe, os.path.join(native, "global_ba_member_check.cc")])
    src = open(os.path.join(native, "global_ba_member_check.cc")).read()
    assert "#define MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT" in src and "Optimizer::GlobalBundleAdjustemnt(pActiveMap, 10, &mbStopGBA, nLoopKF, false);" in src
    syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout
    assert re.search(r" [TW] void ORB_SLAM3::Optimizer::GlobalBundleAdjustemnt<ORB_SLAM3::GBMap>\(ORB_SLAM3::GBMap\*, int, bool\*, unsigned long, bool\)", syms)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "global ba member ok" in out.stdout, out.stdout + out.stderr
