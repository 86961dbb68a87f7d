"""MergeInertialBA without a GPU: the CPU oracle's Jacobians, the oracle pinned to the committed LocalInertialBA oracle, the selection of
the GPU tests' corpus and what its scenes exercise, the header / export pins, and the scratch pins of the kernels it shares."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import merge_inertial_ba_cases as cases
import merge_inertial_ba_oracle as mo
import oracle_lib as O
from morb_slam_amd.synth import _rot_from_rotvec, make_inertial_ba_problem, make_merge_inertial_ba_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _state(rng):
    return np.concatenate([_rot_from_rotvec(rng.normal(0, 0.3, 3)).ravel(), rng.normal(0, 0.5, 3), rng.normal(0, 0.8, 3), rng.normal(0, 0.01, 3),
                           rng.normal(0, 0.05, 3)])


@pytest.mark.parametrize("cam", ["mono", "stereo", "kb8"])
def test_oracle_visual_jacobians_match_central_differences(cam):
    """linearizeOplus of EdgeMono / EdgeStereo in the oracle against central differences of its own computeError, through ImuCamPose's own
    update.  Steps and bars as tests/test_merge_ba_cpu.py documents them: the pinhole monocular edge steps by 1e-4 and agrees within 1e-6 of
    the block's norm; the KannalaBrandt8 projection takes theta and psi from atan2f, so its error moves in steps of ~1e-5 px and it is
    differenced over 1e-2 with a bar of 1e-4, and the stereo edge keeps that step and bar."""
    rng = np.random.default_rng(11)
    p = make_merge_inertial_ba_problem(n_cur=0, n_merge=1, n_cov=0, n_points=20, kb8=cam == "kb8")
    h, bar = (1e-4, 1e-6) if cam == "mono" else (1e-2, 1e-4)
    Tbc = p["Tbc12"].astype(np.float64)
    worst = 0.0
    for _ in range(20):
        s = _state(rng)
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 9)])
        Rwb, twb = s[:9].reshape(3, 3), s[9:12]
        X = Rwb @ (Tbc[:9].reshape(3, 3) @ Xc + Tbc[9:]) + twb          # the point in front of camera 0
        obs = np.array([300.0, 200.0, 280.0 if cam == "stereo" else -1.0], np.float32)
        rows, _, Jp, Jl = mo.vis_edge(p, s, X, obs)
        assert rows == (3 if cam == "stereo" else 2)
        e = lambda s_, X_: mo.vis_edge(p, s_, X_, obs)[1]
        up = lambda k, d: mo.oplus(p["Tbc12"], s, d * np.eye(15)[k])
        Jpn = np.stack([(e(up(k, h), X) - e(up(k, -h), X)) / (2 * h) for k in range(6)], 1)
        Jln = np.stack([(e(s, X + h * np.eye(3)[k]) - e(s, X - h * np.eye(3)[k])) / (2 * h) for k in range(3)], 1)
        for J, Jn in ((Jp, Jpn), (Jl, Jln)):
            assert np.linalg.norm(J) > 1 and not J[rows:].any() and not Jn[rows:].any()
            worst = max(worst, np.abs(J - Jn).max() / np.linalg.norm(J))
    print(cam, "worst difference relative to the block's norm", worst)
    assert worst <= bar


def test_oracle_inertial_jacobian_matches_central_differences():
    """EdgeInertial::linearizeOplus in the oracle against central differences of its computeError through the vertices' own updates.  The
    pose and velocity blocks are smooth FP64: step 1e-4, within 1e-6 of the block's norm.  The bias blocks go through GetDeltaRotation /
    Velocity / Position, float arithmetic on the bias difference (steps of 2^-24 of values near 1, ~1e-7): step 1e-2, bar 1e-4, the pair
    the float-stepped projections take."""
    rng = np.random.default_rng(12)
    p, pre = cases.problem("mix-3x1-s0")
    Tbc = p["Tbc12"]
    worst = {"smooth": 0.0, "bias": 0.0}
    for i in range(len(pre)):
        for _ in range(5):
            s1 = p["true"][p["iKF1"][i]] + np.concatenate([np.zeros(9), rng.normal(0, 0.01, 3), rng.normal(0, 0.02, 3), rng.normal(0, 1e-3, 6)])
            s2 = p["true"][p["iKF2"][i]] + np.concatenate([np.zeros(9), rng.normal(0, 0.01, 3), rng.normal(0, 0.02, 3), np.zeros(6)])
            _, J = mo.inertial_edge(pre[i], s1, s2)
            e = lambda a, b: mo.inertial_edge(pre[i], a, b)[0]
            for c0, n, which, kind in ((0, 6, 1, "smooth"), (6, 3, 1, "smooth"), (9, 6, 1, "bias"), (15, 6, 2, "smooth"), (21, 3, 2, "smooth")):
                h = 1e-4 if kind == "smooth" else 1e-2
                cols = []
                for k in range(n):
                    d = np.zeros(15)
                    d[(c0 if which == 1 else c0 - 15) + k] = h
                    if which == 1:
                        cols.append((e(mo.oplus(Tbc, s1, d), s2) - e(mo.oplus(Tbc, s1, -d), s2)) / (2 * h))
                    else:
                        cols.append((e(s1, mo.oplus(Tbc, s2, d)) - e(s1, mo.oplus(Tbc, s2, -d))) / (2 * h))
                Jn, Jb = np.stack(cols, 1), J[:, c0:c0 + n]
                assert np.linalg.norm(Jb) > 0.1
                worst[kind] = max(worst[kind], np.abs(Jb - Jn).max() / np.linalg.norm(Jb))
    print("worst difference relative to the block's norm", worst)
    assert worst["smooth"] <= 1e-6 and worst["bias"] <= 1e-4


@pytest.mark.parametrize("n_opt,large", [(4, False), (10, False), (4, True), (10, True)])
def test_oracle_with_the_local_plan_is_the_committed_local_inertial_ba_oracle(n_opt, large):
    """Configured as LocalInertialBA — 10 iterations from lambda 1 (bLarge: 4 from 1e-2), its erase rule, the FAIL test, robust kernel and
    information scale per link — the new oracle follows oracle/inertial.cc's orc_local_inertial_ba: same (iterations, trials, ok), same
    erase flags, states and points within 1e-6."""
    p = make_inertial_ba_problem(n_opt=n_opt, n_points=400, seed=n_opt)
    pre = cases.preintegrate(p)
    ok, kfe, mpe, ee, se = O.local_inertial_ba(p, pre, bLarge=large)
    r = mo.run(p, pre, plan=mo.LOCAL_LARGE_PLAN if large else mo.LOCAL_PLAN, local=True)
    assert r["stats3"].tolist() == [int(se[0]), int(se[1]), int(ok)]
    np.testing.assert_array_equal(r["erase"], ee)
    assert np.abs(r["kfState"].astype(np.float64) - kfe).max() <= 1e-6 and np.abs(r["mpPos"].astype(np.float64) - mpe).max() <= 1e-6


def _differ(a, b):
    if a["stats3"].tolist() != b["stats3"].tolist() or (a["erase"] != b["erase"]).any():
        return True
    return max(np.abs(a["kfState"].astype(np.float64) - b["kfState"]).max(), np.abs(a["mpPos"].astype(np.float64) - b["mpPos"]).max()) > 1e-6


def test_corpus_selection():
    """Every case of the GPU corpus through two builds of the oracle (-O2 -ffp-contract=off, points and links in order; -O3
    -ffp-contract=fast, in reverse): a case whose stats or erase flags differ, or whose outputs differ by more than 1e-6, turns on the
    rounding of a sum and is no test of a kernel; it is listed in cases.LEFT_OUT — at most one in ten, never a named scene."""
    differ = [n for n, _ in cases.CASES if _differ(cases.oracle(n), mo.run(*cases.problem(n), flags=mo.OTHER_FLAGS))]
    print("cases that differ between the two builds:", differ)
    assert set(differ) <= set(cases.LEFT_OUT), differ
    assert set(cases.LEFT_OUT) <= {n for n, _ in cases.CASES} and len(cases.LEFT_OUT) * 10 <= len(cases.CASES)
    assert not set(cases.LEFT_OUT) & set(cases.NAMED_NAMES)


def _free_counts(p):
    return int((p["kfKind"] == 0).sum()), int((p["kfKind"] == 3).sum())


def test_corpus_coverage():
    """Cameras mix / mono / kb8 at every (15-dof, 6-dof) size of the table — P = 30, 51, 162 (last on the LDS-resident LDL^T), 165 twice
    (first on the global-memory solver), 375 with 300 points —, 60 or 300 points elsewhere, and the chunk-edge scenes."""
    seen = {}
    for name, kw in cases.CASES:
        if name not in cases.KEPT or name in cases.NAMED_NAMES:
            continue
        p, _ = cases.problem(name)
        cam = name.split("-")[0]
        seen.setdefault((cam, _free_counts(p)), []).append(kw["n_points"])
        mono = p["eObs"][:, 2] < 0
        assert kw["n_points"] in (60, 300)
        assert mono.all() if cam in ("mono", "kb8") else (mono.any() and (~mono).any())
        assert (p["rig28"] is not None) == (cam == "kb8")
    for cam in cases.CAMERAS:
        for n15n6 in cases.SIZES:
            assert (cam, n15n6) in seen, (cam, n15n6)
        assert 300 in seen[(cam, (13, 30))]
    assert [15 * a + 6 * b for a, b in cases.SIZES] == [30, 51, 162, 165, 165, 375]
    for name, want in (("chunk63", 63), ("chunk64", 64), ("chunk65", 65)):
        assert name in cases.KEPT
        p, _ = cases.problem(name)
        counts = np.bincount(p["eKF"], minlength=len(p["kfKind"]))
        assert counts[1] == counts[4] == want and p["kfKind"][1] == 0 and p["kfKind"][4] == 3


def test_scene_power():
    """Asserted on the oracle alone: the corpus holds rejected trials, a solve that runs all 8 iterations, a link whose initial chi2 exceeds
    16.92 (Huber weight below 1), erased mono and stereo edges, a mono edge with negative depth and chi2 under the bar that is NOT erased, a
    point seen only by pose-only keyframes, and a chain A of one keyframe (a free head with no link)."""
    for n in cases.NAMED_NAMES:
        assert n in cases.KEPT
    r = cases.oracle("shifted-fixed")
    assert r["stats3"][1] > r["stats3"][0] == 8              # trials were rejected on the way, and all 8 iterations ran
    assert cases.oracle("mix-10x2-s0")["stats3"].tolist() == [8, 8, 1]
    r = cases.oracle("kicked-link")
    assert (r["linkChi0"] > 16.92).any()
    (p, _), r = cases.problem("mix-9x5-s1"), cases.oracle("mix-9x5-s1")
    mono = p["eObs"][:, 2] < 0
    assert r["erase"][mono].sum() > 0 and r["erase"][~mono].sum() > 0
    for name in ("behind", "behind-kb8"):
        (p, _), r = cases.problem(name), cases.oracle(name)
        kept_behind = (r["depthEnd"] < 0) & (r["chiEnd"] <= np.float32(5.991)) & (r["erase"] == 0)
        assert kept_behind.sum() >= 1 and (p["mpTag"][p["eMP"][kept_behind]] == 1).all() and (p["eObs"][kept_behind, 2] < 0).all()
        assert (r["erase"][r["depthEnd"] < 0] == (r["chiEnd"][r["depthEnd"] < 0] > np.float32(5.991))).all()     # chi2 alone decides
    p, _ = cases.problem("cov-only-points")
    lonely = [m for m in np.where(p["mpTag"] == 2)[0] if (p["kfKind"][p["eKF"][p["eMP"] == m]] == 3).all()]
    assert len(lonely) >= 1 and len(lonely) == int((p["mpTag"] == 2).sum())
    p, _ = cases.problem("single-head")
    assert p["kfKind"][0] == 0 and not (p["iKF1"] == 0).any() and not (p["iKF2"] == 0).any() and _free_counts(p) == (2, 0)
    p, _ = cases.problem("observers")
    assert set(p["kfKind"].tolist()) == {0, 1, 2, 3}


def test_scene_power_of_the_lm_endings():
    """Asserted on the oracle alone: a solve that ENDS on a rejected trial, and solves the stagnation rule ends before the 8th iteration.
    From setUserLambdaInit(1e3) the damped steps of an ordinary scene gain more than 0.1 % in every one of the 8 iterations and every
    iteration's last trial is accepted, so both scenes carry a link between two fixed keyframes — a constant of the robust chi2 — far enough
    apart (merge_inertial_ba_cases.NAMED says how far, and why)."""
    r = cases.oracle("ends-rejected")
    assert r["info4"][0] == 1 and r["stats3"].tolist() == [1, 1, 1]
    p, _ = cases.problem("ends-rejected")
    assert r["kfState"].tobytes() == p["kfState"].tobytes() and r["mpPos"].tobytes() == p["mpPos"].tobytes()   # the rejected step was undone
    for name in ("stagnates", "stagnates-kb8"):
        r = cases.oracle(name)
        assert r["info4"].tolist()[:2] == [0, 1] and r["stats3"][0] == 3 and r["stats3"][2] == 1
        p, _ = cases.problem(name)
        assert (p["kfKind"] == 1).sum() == 2 and np.isin(p["iKF1"], np.where(p["kfKind"] == 1)[0]).sum() == 2
        assert not np.array_equal(r["kfState"], p["kfState"])                                                      # (it did move before it stalled)


def test_stop_plan_of_the_oracle():
    p, pre = cases.problem("mix-3x1-s0")
    r = mo.run(p, pre, stop_entry=True)
    assert r["stats3"].tolist() == [0, 0, 0] and r["kfState"].tobytes() == p["kfState"].tobytes() and not r["erase"].any()


def test_header_declares_and_library_exports_the_entries():
    from morb_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_merge_inertial_ba\(morb_optimizer\*, int nKF, float\* kfState21, const uint8_t\* kfKind, int nMP, float\* mpPos,", header)
    assert "Optimizer.cc:3853-4389" in header and "LoopClosing.cc:1649-1650" in header and ":2099" in header
    for word in (":3856-3983", "SetNewBias", "UpdateNormalAndDepth", "corrPoses"):
        assert word in header
    for name, nargs in (("morb_merge_inertial_ba", 24), ("morb_merge_inertial_ba_fisheye", 20)):
        restype, argtypes = capi.HEADER.prototypes[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("library not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.lib()
    for name in ("morb_merge_inertial_ba", "morb_merge_inertial_ba_fisheye"):
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert list(getattr(L, name).argtypes) == capi.HEADER.prototypes[name][1]     # the parsed prototype went through capi.py's loop


def test_the_shared_kernels_keep_their_scratch_pins(tmp_path):
    """MergeInertialBA adds no kernel: it runs LocalInertialBA's k_iba_* with a column table.  The unit declares the kernels it declared
    before, and every one of them keeps the scratch use tests/test_codeobj_cpu.py pins: zero but for k_iba_errors <= 68 and k_iba_kf <= 84
    (the other k_iba_* kernels, which that file does not list, are held to zero here)."""
    import test_codeobj_cpu as co
    src = open(os.path.join(ROOT, "morb_slam_amd", "csrc", "inertial_ba.hip")).read()
    declared = set(re.findall(r"__global__[^\n]*?void (k_iba_\w+)\(", src))
    assert declared == {"k_iba_setup_kf", "k_iba_setup_pts", "k_iba_setup_links", "k_iba_errors", "k_iba_end", "k_iba_lm_init", "k_iba_points",
                        "k_iba_kf", "k_iba_links", "k_iba_pack_w", "k_iba_pack_wd", "k_iba_schur_finish", "k_iba_solve_lds",
                        "k_iba_solve_blocked", "k_iba_update", "k_iba_finish"}
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    if not (os.path.exists(lib) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(lib, str(tmp_path)).items() if "k_iba_" in k}
    found = set()
    for mangled, scratch in meta.items():
        name = max((d for d in declared if re.search(r"\d+" + d + r"(E|I)", mangled)), key=len)
        found.add(name)
        assert scratch <= {"k_iba_errors": 68, "k_iba_kf": 84}.get(name, 0), (mangled, scratch)
    assert found == declared


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/merge_inertial_ba_member_check.cc: the call expression of LoopClosing.cc:1649-1650 unedited, window and covisible selection,
    kinds, links, marks, write-back and corrPoses against hand-built expectations, with the C entries stubbed in the program; built with
    -fsanitize=address,undefined as a stand-alone program."""
    exe = str(tmp_path / "merge_inertial_ba_member_check")
    src_path = os.path.join(NATIVE, "merge_inertial_ba_member_check.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(NATIVE, "mock_merge_inertial_ba"), "-I" + os.path.join(NATIVE, "mock_ref"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, src_path])
    src = open(src_path).read()
    assert "Optimizer::MergeInertialBA(mpCurrentKF, mpMergeMatchedKF, &bStop,\n                               pCurrentMap, vCorrectedSim3);" in src
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "merge inertial ba member ok" in out.stdout, out.stdout + out.stderr
