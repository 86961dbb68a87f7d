"""The welding bundle adjustment of map merging without a GPU: the CPU oracle's Jacobians, the oracle pinned to the committed
LocalBundleAdjustment oracle, the selection of the GPU tests' corpus and what its scenes exercise, the header / export pins, and the
reference-typed member on a mock map under sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import merge_ba_cases as cases
import merge_ba_oracle as mo
import oracle_lib as O
from morb_slam_amd.synth import EUROC_CAM, TUMVI_CAM_L, _rot_from_rotvec, make_ba_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("cam", ["mono", "stereo", "kb8"])
def test_oracle_jacobians_match_central_differences(cam):
    """linearizeOplus of the oracle's three edges against central differences of its own computeError, through the vertices' own updates
    (SE3Quat::exp(u) * T for the pose): 20 points under random poses.  Bars as in tests/test_initial_map_cpu.py: the pinhole monocular edge
    steps by 1e-4 and agrees within 1e-6 of the block's norm; the KannalaBrandt8 projection takes theta and psi from atan2f, so its error
    moves in steps of ~1e-5 px and it is differenced over 1e-2 with a bar of 1e-4; the stereo edge divides by a FLOAT 1 / z (cam_project's
    `const float invz`): steps of 2^-24 * 450 px = 3e-5 px, the same step and bar as KannalaBrandt8."""
    rng = np.random.default_rng(5)
    kb8 = cam == "kb8"
    cam8 = TUMVI_CAM_L if kb8 else np.array([EUROC_CAM[k] for k in ("fx", "fy", "cx", "cy", "bf")] + [0, 0, 0], np.float32)
    h, bar = (1e-4, 1e-6) if cam == "mono" else (1e-2, 1e-4)
    worst = 0.0
    for _ in range(20):
        T = np.concatenate([_rot_from_rotvec(rng.normal(0, 0.2, 3)).ravel(), rng.normal(0, 0.3, 3)])
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 9)])
        X = T[:9].reshape(3, 3).T @ (Xc - T[9:])
        obs = np.array([300.0, 200.0, 280.0 if cam == "stereo" else -1.0], np.float32)
        rows, _, Jp, Jl = mo.edge(kb8, cam8, T, X, obs)
        assert rows == (3 if cam == "stereo" else 2)
        e = lambda T_, X_: mo.edge(kb8, cam8, T_, X_, obs)[1]
        Jpn = np.stack([(e(mo.oplus(T, h * np.eye(6)[k]), X) - e(mo.oplus(T, -h * np.eye(6)[k]), X)) / (2 * h) for k in range(6)], 1)
        Jln = np.stack([(e(T, X + h * np.eye(3)[k]) - e(T, X - h * np.eye(3)[k])) / (2 * h) for k in range(3)], 1)
        for J, Jn in ((Jp, Jpn), (Jl, Jln)):
            assert np.linalg.norm(J) > 1 and not J[rows:].any() and not Jn[rows:].any()
            worst = max(worst, np.abs(J - Jn).max() / np.linalg.norm(J))
    print(cam, "worst difference relative to the block's norm", worst)
    assert worst <= bar


@pytest.mark.parametrize("kw", [dict(seed=1), dict(seed=2, n_free=8, n_fixed=3, n_points=500), dict(seed=3, n_free=20, n_fixed=6, n_points=3000, mono_frac=0.5)])
def test_oracle_as_one_robust_round_is_the_committed_local_ba_oracle(kw):
    """Configured as LocalBundleAdjustment — one robust round of ten iterations, delta^2 5.991 — the new oracle follows oracle/optimizer.cc's
    orc_local_ba on the problems of tests/test_optimizer_gpu.py: same (iterations, trials), same erase flags, poses and points within 1e-6."""
    b = make_ba_problem(**kw)
    for lam in (False, True):
        _, kfe, mpe, ee, se = O.local_ba(b, lambda100=lam)
        r = mo.run(b, plan=mo.LOCAL_BA_PLAN, user_lambda=100.0 if lam else 0.0)
        assert r["stats6"].tolist() == [int(se[0]), int(se[1]), 0, 0, 0, 1]
        np.testing.assert_array_equal(r["erase"], ee)
        assert np.abs(r["kfPose"].astype(np.float64) - kfe).max() <= 1e-6 and np.abs(r["mpPos"].astype(np.float64) - mpe).max() <= 1e-6
        assert not r["level"].any()


def _differ(a, b):
    if a["stats6"].tolist() != b["stats6"].tolist() or (a["level"] != b["level"]).any() or (a["erase"] != b["erase"]).any():
        return True
    return max(np.abs(a["kfPose"].astype(np.float64) - b["kfPose"]).max(), np.abs(a["mpPos"].astype(np.float64) - b["mpPos"]).max()) > 1e-6


def test_corpus_selection():
    """Every case of the GPU corpus through two builds of the oracle (-O2 -ffp-contract=off, points in order; -O3 -ffp-contract=fast, points in
    reverse): a case whose stats, level or erase flags differ, or whose outputs differ by more than 1e-6, turns on the rounding of a sum and is
    no test of a kernel; it is listed in cases.LEFT_OUT — at most one in ten."""
    differ = [c for c in cases.CASES if _differ(cases.case_oracle(c), cases.case_oracle(c, mo.OTHER_FLAGS))]
    print("cases that differ between the two builds:", differ)
    assert set(differ) <= cases.LEFT_OUT, differ
    assert cases.LEFT_OUT <= set(cases.CASES) and len(cases.LEFT_OUT) * 10 <= len(cases.CASES)


def test_corpus_covers_the_grid():
    kept = [c for c in cases.CASES if c not in cases.LEFT_OUT]
    assert {c[:4] for c in kept} >= {(cam, f, x, n) for cam in cases.CAMS for f in (1, 3, 27, 28) for x in (1, 4) for n in (60, 300)}
    for c in cases.CHUNK_EDGE:
        assert c in kept
        counts = np.bincount(cases.scene(c)["eKF"])
        assert counts[:3].tolist() == [63, 64, 65]
    for c in kept:   # both rounds run everywhere, and a "mix" scene has both kinds of edge
        p = cases.scene(c)
        assert cases.case_oracle(c)["stats6"][5] == 2
        if c[0] == "mix":
            assert (p["eObs"][:, 2] < 0).any() and (p["eObs"][:, 2] >= 0).any()
        if c[0] == "mono":
            assert (p["eObs"][:, 2] < 0).all()


def test_scene_power():
    """Asserted on the oracle alone: the corpus holds a round 1 that ends on a rejected trial, a point and a free keyframe that lose all their
    edges to level 1, and an edge erased on its stale chi2 although its chi2 at the final estimate passes."""
    for c in cases.NAMED:
        assert c not in cases.LEFT_OUT
    r = cases.case_oracle(cases.REJECTED_LAST)
    assert r["info4"][0] == 1 and r["stats6"][5] == 2
    r = cases.case_oracle(cases.POINT_DROPS)
    assert r["info4"][1] >= 1
    p = cases.scene(cases.POINT_DROPS)
    lost = [m for m in range(len(p["mpPos"])) if (p["eMP"] == m).any() and r["level"][p["eMP"] == m].all()]
    assert len(lost) == r["info4"][1]
    r, p = cases.case_oracle(cases.KEYFRAME_DROPS), cases.scene(cases.KEYFRAME_DROPS)
    assert r["info4"][2] >= 1 and r["level"][p["eKF"] == 1].all() and not p["kfFixed"][1]
    r, p = cases.case_oracle(cases.STALE_CHI2), cases.scene(cases.STALE_CHI2)
    thr = np.where(p["eObs"][:, 2] < 0, 5.991, 7.815)
    stale_only = (r["level"] != 0) & (r["erase"] != 0) & (r["chiStale"] > thr) & (r["chiFresh"] <= thr)
    assert stale_only.sum() == r["info4"][3] >= 1
    assert (p["eKF"][stale_only] == 2).any()          # among them edges of the keyframe whose own pose error round 1 did not remove
    print("edges erased on the stale chi2 alone:", int(stale_only.sum()), "of", int(r["erase"].sum()), "erased")


def test_stop_plans_of_the_oracle():
    p = cases.scene(cases.GRID[6])
    full = mo.run(p)
    r = mo.run(p, stop_entry=True)
    assert r["stats6"].tolist() == [0] * 6 and r["kfPose"].tobytes() == p["kfPose"].tobytes() and not r["erase"].any()
    r = mo.run(p, stop_after=1)
    assert r["stats6"].tolist() == full["stats6"][:2].tolist() + [0, 0, 0, 1] and not r["level"].any()


def test_header_declares_and_library_exports_the_entries():
    from morb_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_merge_bundle_adjustment\(morb_optimizer\*, int nKF, float\* kfPose, const uint8_t\* kfFixed, int nMP, float\* mpPos,", header)
    assert "Optimizer.cc:3430-3851" in header and "LoopClosing.cc:1652" in header
    for name, nargs in (("morb_merge_bundle_adjustment", 20), ("morb_merge_bundle_adjustment_fisheye", 16)):
        restype, argtypes = capi.HEADER.prototypes[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("library not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.lib()
    for name in ("morb_merge_bundle_adjustment", "morb_merge_bundle_adjustment_fisheye"):
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert list(getattr(L, name).argtypes) == capi.HEADER.prototypes[name][1]     # the parsed prototype went through capi.py's loop


def test_kernels_use_no_scratch_memory(tmp_path):
    import test_codeobj_cpu as co
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    if not (os.path.exists(lib) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(lib, str(tmp_path)).items() if re.search(r"\d+k_mg_(chi2|build|finish|reset)(I|E)", k)}
    assert len(meta) == 5, meta          # k_mg_build in its pinhole and KannalaBrandt8 forms
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/merge_ba_member_check.cc: the call expression of LoopClosing.cc:1652-1653 unedited, graph selection, marks and write-back
    against hand-built expectations, with the C entries stubbed in the program; built with -fsanitize=address,undefined as a stand-alone program."""
    exe = str(tmp_path / "merge_ba_member_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(NATIVE, "mock_merge_ba"), "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "merge_ba_member_check.cc")])
    src = open(os.path.join(NATIVE, "merge_ba_member_check.cc")).read()
    assert "Optimizer::LocalBundleAdjustment(mpCurrentKF, vpLocalCurrentWindowKFs,\n                                     vpMergeConnectedKFs, &bStop);" in src
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "merge ba member ok" in out.stdout, out.stdout + out.stderr
