"""The numeric part of Tracking::CreateInitialMapMonocular without a GPU: the CPU oracle's Jacobians and its ability to solve the problem,
the selection of the GPU tests' corpus, the shared host / device arithmetic under sanitizers, the reference-typed members' instantiation
and their refusal of other map shapes, the header / export / scratch pins."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import initial_map_cases as cases
import initial_map_oracle as io
from morb_slam_amd.synth import _rot_from_rotvec, make_initial_map_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("cam", cases.CAMS)
def test_oracle_jacobians_match_central_differences(cam):
    """EdgeSE3ProjectXYZ::linearizeOplus of the oracle against central differences of its own computeError, through the vertices' own updates
    (SE3Quat::exp(u) * T for the pose): 20 points under perturbed poses.  Pinhole: step 1e-4, 1e-6 of the block's norm.  KannalaBrandt8's
    projection takes theta and psi from atan2f (the reference's float leak): the error steps by ~2^-24 * 190 px = 1e-5 px, which a
    difference over 2 h = 2e-2 turns into 1e-3 px per unit at most, so its step is 1e-2 and its bar 1e-4 of the norm (the norms are 30 .. 200; a
    sign, a transposition or a misplaced block is of order one)."""
    p = make_initial_map_problem(seed=2, n_points=30, cam=cam)
    rng = np.random.default_rng(3)
    h, bar = (1e-2, 1e-4) if cam == "kb8" else (1e-4, 1e-6)
    worst = 0.0
    for i in np.nonzero(p["triangulated"])[0][:20]:
        X = p["X_true"][i] * (1 + rng.normal(0, 0.05))
        obs = p["kp2"][p["matches12"][i], :2].astype(np.float64)
        T = np.concatenate([(_rot_from_rotvec(rng.normal(0, 0.1, 3)) @ p["T21_true"][:9].reshape(3, 3)).ravel(), p["T21_true"][9:] + rng.normal(0, 0.05, 3)])
        e = lambda T_, X_: io.edge(p["kb8"], p["cam8"], T_, X_, obs)[0]
        _, Jp, Jl = io.edge(p["kb8"], p["cam8"], T, X, obs)
        Jpn = np.stack([(e(io.oplus(T, h * np.eye(6)[k]), X) - e(io.oplus(T, -h * np.eye(6)[k]), X)) / (2 * h) for k in range(6)], 1)
        Jln = np.stack([(e(T, X + h * np.eye(3)[k]) - e(T, X - h * np.eye(3)[k])) / (2 * h) for k in range(3)], 1)
        for J, Jn in ((Jp, Jpn), (Jl, Jln)):
            assert np.linalg.norm(J) > 1
            worst = max(worst, np.abs(J - Jn).max() / np.linalg.norm(J))
    print(cam, "worst difference relative to the block's norm", worst)
    assert worst <= bar


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_oracle_recovers_truth_on_noise_free_data(scale):
    """Noise-free observations, points and pose perturbed: 20 iterations bring chi2 to zero.  The cost does not see the scale of the scene,
    so the truth is compared after the same normalisation: the scaled median depth of keyframe 1 is depthScale (1, or 4 for IMU-monocular),
    and pose and points equal the truth scaled to that median within 1e-4 (float outputs at depths of 0.5 .. 7)."""
    p = make_initial_map_problem(seed=1, n_points=150, noise_px=0.0, n_untriangulated=0, point_noise=0.03, pose_noise=(0.01, 0.03))
    r = io.run(p, 20, True, depthScale=scale)
    print("stats", r["stats"], "chi2", r["chi2"], "median", r["median"])
    assert r["status"] == 1 and r["chi2"][0] > 100 and r["chi2"][1] < 1e-6
    m = r["hasMP"] != 0
    assert m.sum() == 150
    z = np.sort(r["mpPos"][m, 2])
    assert abs(z[(len(z) - 1) // 2] - scale) <= 1e-5 * scale
    zt = np.sort(p["X_true"][m, 2])
    s = scale / zt[(len(zt) - 1) // 2]
    assert np.abs(r["mpPos"][m] - p["X_true"][m] * s).max() <= 1e-4 * scale
    assert np.abs(r["Tcw2"][:9] - p["T21_true"][:9]).max() <= 1e-5 and np.abs(r["Tcw2"][9:] - p["T21_true"][9:] * s).max() <= 1e-4 * scale


def _worst(a, b):
    return max(np.abs(a[k].astype(np.float64) - b[k]).max() if a[k].size else 0.0 for k in ("Tcw2", "mpPos", "mpNormal", "mpDist"))


def test_corpus_selection():
    """Every case of the GPU corpus through two builds of the oracle (-O2 -ffp-contract=off, points in order; -O3 -ffp-contract=fast, points in
    reverse): a case whose (iterations, trials) differ, or whose outputs differ by more than 1e-6 on the same path, turns on the rounding of a
    sum and is no test of a kernel; it is listed in cases.LEFT_OUT — at most one in ten.  A kept case also keeps the scale it started with
    within a factor two (see cases.scene)."""
    differ = []
    for c in cases.CASES:
        a, b = cases.case_oracle(c), cases.case_oracle(c, io.OTHER_FLAGS)
        if a["stats"].tolist() != b["stats"].tolist() or a["status"] != b["status"] or _worst(a, b) > 1e-6:
            differ.append(c)
        elif c not in cases.LEFT_OUT:
            start = cases.case_oracle(c[:2] + (0,) + c[3:])["median"]
            assert 0.5 * start < a["median"] < 2 * start, (c, start, a["median"])
    print("cases that differ between the two builds:", differ)
    assert set(differ) <= cases.LEFT_OUT, differ
    assert len(cases.LEFT_OUT) * 10 <= len(cases.CASES)


def test_other_scenes_do_not_turn_on_rounding():
    """The outlier, mixed-batch, stop, scale and LocalBundleAdjustment scenes of the GPU tests, the same two builds."""
    todo = [(cases.outlier_scene(), dict(nIterations=20, robust=0))]
    for seed, kw in ((40, dict(n_points=120)), (41, dict(n_points=30)), (42, dict(n_points=90, behind=True)), (43, dict(n_points=300, outlier_frac=0.05)),
                     (45, dict(n_points=257)), (50, dict(n_points=100)), (51, dict(n_points=100)), (60, dict(n_points=130))):
        todo.append((make_initial_map_problem(seed=seed, **kw), dict(nIterations=20, robust=1)))
    for n in (60, 300):
        todo.append((make_initial_map_problem(seed=300 + n, n_points=n, noise_px=0.5, outlier_frac=0.04), dict(nIterations=10, robust=1, depthScale=0.0)))
    for k, (p, kw) in enumerate(todo):
        a, b = io.run(p, **kw), io.run(p, flags=io.OTHER_FLAGS, **kw)
        assert a["stats"].tolist() == b["stats"].tolist() and a["status"] == b["status"] and _worst(a, b) <= 1e-6, (k, a["stats"], b["stats"], _worst(a, b))


def test_shared_arithmetic_under_sanitizers(tmp_path):
    """tests/native/initial_map_math_check.cc: the depth keys, the selection of the median by bits against a sort (n = 1 .. 70, ties, both
    zeros, negative depths), the status bits, the scaling, the camera centre and UpdateNormalAndDepth's fields; built with
    -fsanitize=address,undefined as a stand-alone program."""
    exe = str(tmp_path / "initial_map_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(NATIVE, "initial_map_math_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "initial map math ok" in out.stdout, out.stdout + out.stderr


def test_reference_typed_members_instantiate_and_refuse_other_maps(tmp_path):
    """GlobalBundleAdjustemnt(Map*, int, bool*, unsigned long, bool) and BundleAdjustment(vpKFs, vpMP, ...) compile against the mock map
    (tests/native/mock_initial_map) with the call site's argument list, the program holds both, and a map of three keyframes is refused
    with std::runtime_error before any device call (so this runs without a GPU)."""
    exe = str(tmp_path / "initial_map_member_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    if not os.path.exists(os.path.join(libdir, "libmorb_hip.so")):
        pytest.skip("library not built")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_initial_map"), "-I" + os.path.join(ROOT, "include", "morb"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, os.path.join(NATIVE, "initial_map_member_check.cc"),
                           "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout
    assert re.search(r" [TW] void ORB_SLAM3::Optimizer::GlobalBundleAdjustemnt<ORB_SLAM3::IMMap>\(ORB_SLAM3::IMMap\*, int, bool\*, unsigned long, bool\)", syms), syms
    assert re.search(r" [TW] void ORB_SLAM3::Optimizer::BundleAdjustment<ORB_SLAM3::IMKeyFrame, ORB_SLAM3::IMMapPoint>\(", syms), syms
    out = subprocess.run([exe, "refusals"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "three keyframes refused" in out.stdout and "stereo observation refused" in out.stdout, out.stdout + out.stderr


def test_header_declares_and_library_exports_the_entry():
    from morb_slam_amd.capi import HEADER
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_create_initial_map_monocular_batch\(morb_optimizer\*, const morb_frame_params\* P, const float\* cam8, int kb8, int nprob, int cap,",
                     header)
    assert "morb_create_initial_map_monocular_batch" in HEADER.prototypes
    if not os.path.exists(lib):
        pytest.skip("library not built")
    assert hasattr(ctypes.CDLL(lib), "morb_create_initial_map_monocular_batch")


def test_kernel_scratch_is_pinned(tmp_path):
    """k_initial_map in its four forms (pinhole / KannalaBrandt8, records in LDS / in the workspace) uses no scratch memory (DESIGN.md section 6,
    "Initial map")."""
    import test_codeobj_cpu as co
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    if not (os.path.exists(lib) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(lib, str(tmp_path)).items() if "k_initial_mapI" in k}
    assert len(meta) == 4, meta
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)
    for pats in (co.HOT, co.BOUNDED):   # the name stays clear of the lists of tests/test_codeobj_cpu.py
        assert not any(re.search(r"\d+" + short + r"(I|E)", k) for short in pats for k in meta)
