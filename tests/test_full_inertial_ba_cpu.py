"""The inertial whole-map bundle adjustment without a GPU: the skyline oracle pinned to the dense inertial oracle already in the tree, the
first system of bInit against a finite-difference gradient, the selection of the GPU tests' corpus and what its scenes exercise, the header /
export pins and the kernels' scratch memory."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import full_inertial_ba_cases as cases
import full_inertial_ba_oracle as fo
import merge_inertial_ba_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_PINHOLE = [c for c in cases.CASES if not dict(c[1]).get("init") and not dict(c[1]).get("kb8")]
PLAIN_RIG = [c for c in cases.CASES if not dict(c[1]).get("init") and dict(c[1]).get("kb8")]


def _merge_oracle(case):
    p, pre = cases.scene(case)
    return mo.run(p, pre, plan=dict(iterations=case[2], lambda0=1e-5, erase_chi2_only=True, fail_test=False))


@pytest.mark.parametrize("case", PLAIN_PINHOLE, ids=cases.case_id)
def test_oracle_is_the_dense_inertial_oracle_on_pinhole_cases(case):
    """tests/native/merge_inertial_ba_oracle.cc with FullInertialBA's plan (optimize(its) from lambda 1e-5, erase by chi2 alone, no FAIL
    test) is this function on a pinhole map without bInit: the same edges into a dense reduced system.  A skyline only skips exact zeros:
    states, points and (iterations, trials) are equal bit for bit — on every case whose gauge is fixed but the largest, where the dense
    oracle's pivoting shows in the last places of some floats (1.5e-7; held to 1e-6, the corpus selection's bound).  Where nothing is fixed they cannot
    be: the dense oracle's Eigen-style LDL^T pivots on the diagonal, the skyline one cannot, and the four gauge directions of the system
    are held by lambda = 1e-5 alone, so the two orders of the same sums part in the low bits of the float outputs (measured: at most 1.5e-5,
    small-mono-3kf-init0; tests/full_inertial_ba_cases.py and profiles/r20/README.md).  The issue's bit-for-bit requirement cannot be met on
    those cases; they are held to the LM path and to 3e-5, twice the measured figure.  That the skyline itself changes nothing is shown
    exactly by test_skyline_skips_nothing_but_exact_zeros."""
    a, m = cases.case_oracle(case), _merge_oracle(case)
    assert a["stats4"][:2].tolist() == m["stats3"][:2].tolist()
    if dict(case[1]).get("n_fixed"):
        if case == cases.GAUGED_LARGE:   # 1785 unknowns: the dense oracle's pivoting reorders enough of the sums to show in the floats' last places
            same, d = cases.parting(a, dict(m, bias6=a["bias6"], stats4=a["stats4"]))
            print(case[0], "apart", d, "floats that differ", int((a["kfState"] != m["kfState"]).sum() + (a["mpPos"] != m["mpPos"]).sum()))
            assert d <= 1e-6
        else:
            assert a["kfState"].tobytes() == m["kfState"].tobytes() and a["mpPos"].tobytes() == m["mpPos"].tobytes()
    else:
        same, d = cases.parting(a, dict(m, bias6=a["bias6"], stats4=a["stats4"]))
        print(case[0], "apart", d)
        assert d <= 3e-5


@pytest.mark.parametrize("case", PLAIN_RIG, ids=cases.case_id)
def test_oracle_follows_the_dense_inertial_oracle_on_rig_cases(case):
    """On the rig a keyframe sees a point through two edges (left and right camera): both oracles add every (edge, edge) product of the
    Schur complement on its own, in the same order, so the rig cases can be held exactly as the pinhole ones are: bit for bit where the
    gauge is fixed, the LM path and 3e-5 where it is not.  (The dense oracle runs with LocalInertialBA's arrays, which carry eRight.)"""
    a, m = cases.case_oracle(case), _merge_oracle_rig(case)
    assert a["stats4"][:2].tolist() == m["stats3"][:2].tolist()
    if dict(case[1]).get("n_fixed"):
        assert a["kfState"].tobytes() == m["kfState"].tobytes() and a["mpPos"].tobytes() == m["mpPos"].tobytes()
    else:
        same, d = cases.parting(a, dict(m, bias6=a["bias6"], stats4=a["stats4"]))
        print(case[0], "apart", d)
        assert d <= 3e-5


def _merge_oracle_rig(case):
    p, pre = cases.scene(case)
    q = dict(p, mpClose=np.zeros(len(p["mpPos"]), np.uint8), iRobust=np.ones(max(len(p["iKF1"]), 1), np.uint8),
             iInfoScale=np.ones(max(len(p["iKF1"]), 1), np.float32))
    return mo.run(q, pre, plan=dict(iterations=case[2], lambda0=1e-5, erase_chi2_only=True, fail_test=False), local=True)


# The finite-difference errors to expect, measured on the !bInit scene, whose system is pinned to the dense oracle: the largest
# |-2 b - gradient| / max(1, |gradient|) at step 1e-4 over the pose, velocity and point unknowns (measured 2.1e-5) and over the bias unknowns
# (measured 4.0e-2: the preintegrated deltas are floats, ImuTypes.cc:289-312, so the error of a link is a staircase in the bias with steps of
# ~3e-8 under informations of ~1e5, and a difference quotient across 2e-4 sees the steps).  bInit is held to ten times each.
FD_STEP = 1e-4
FD_ERROR_PLAIN = 2.5e-5
FD_ERROR_PLAIN_BIAS = 4.5e-2
_AT_TRUTH = dict(n_kf=6, reach=3, n_points=60, seed=900, n_imu=cases.N_IMU, at_truth=True)   # no edge above its Huber bar: rho' = 1 everywhere


def _gradient_errors(init):
    from morb_slam_amd.synth import make_full_inertial_ba_problem
    p = make_full_inertial_ba_problem(init=init, **_AT_TRUTH)
    pre = cases.preintegrate(p)
    P, b, g, above = fo.gradient(p, pre, h=FD_STEP)
    assert not above and P == (6 * 9 + 6 if init else 6 * 15)
    err = np.abs(-2 * b - g) / np.maximum(1.0, np.abs(g))
    bias = np.zeros(len(err), bool)
    if init:
        bias[P - 6:P] = True
    else:
        bias[:P] = np.arange(P) % 15 >= 9
    return err[~bias].max(), err[bias].max(), g[bias]


def test_first_system_of_binit_is_the_gradient():
    """No earlier oracle has shared bias vertices.  On a scene where no edge is above its Huber bar, -2 b of the first system equals the
    central-difference gradient of the oracle's own robust chi2 along every unknown — the nine of every keyframe, the six shared ones, the
    points.  The same check on the !bInit scene, whose system is pinned to the dense oracle, measures the finite-difference error to
    expect: 2.1e-5 away from the biases, 4.0e-2 on them.  bInit is held to ten times that; measured 2.1e-5 and, on the shared six, 1.4e-4
    (their gradient is ~1e5: a prior with the wrong sign would be an error of order one)."""
    plain, plain_bias, _ = _gradient_errors(False)
    init, init_bias, g = _gradient_errors(True)
    print("!bInit: largest relative gradient error", plain, "on the biases", plain_bias, "| bInit:", init, "on the shared six", init_bias,
          "whose gradient is", g)
    assert plain <= FD_ERROR_PLAIN and plain_bias <= FD_ERROR_PLAIN_BIAS
    assert init <= 10 * FD_ERROR_PLAIN and init_bias <= 10 * FD_ERROR_PLAIN_BIAS
    assert np.abs(g).min() > 1e3          # the shared unknowns do carry a gradient: the links and the priors pull on them


def test_skyline_skips_nothing_but_exact_zeros():
    """The oracle built with -DFIB_ORACLE_DENSE factorises the whole lower triangle, without pivoting, with the same arithmetic: every case
    of the corpus gives the same bytes and the same stats, free gauge or not.  (The dense oracle of MergeInertialBA pivots on the diagonal;
    that, not the skyline, is what parts the two above where nothing is fixed.)"""
    for c in cases.CASES + cases.FREE_PATH + cases.LONE:
        if len(cases.scene(c)[0]["kfState"]) > 40:
            continue   # (the two 120-keyframe scenes: a dense factor of 1800 rows adds nothing the 30-keyframe ones do not show)
        a, d = cases.case_oracle(c), cases.case_oracle(c, fo.DENSE_FLAGS)
        assert a["stats4"].tolist() == d["stats4"].tolist() and a["chi2"].tobytes() == d["chi2"].tobytes(), c[0]
        assert a["kfState"].tobytes() == d["kfState"].tobytes() and a["mpPos"].tobytes() == d["mpPos"].tobytes() and a["bias6"].tobytes() == d["bias6"].tobytes(), c[0]


def test_call_site_configuration_spreads():
    """Nothing fixed, 7 and 100 iterations: the figures the device is held to, measured between the oracle's two builds and pinned."""
    spread = gap = 0.0
    for c in cases.FREE_PATH:
        (p, pre), a, b = cases.scene(c), cases.case_oracle(c), cases.case_oracle(c, fo.OTHER_FLAGS)
        assert not np.isin(p["kfKind"], (1, 2)).any() and c[2] in (7, 100) and a["stats4"][0] > 1 and a["chi2"][1] < a["chi2"][0]
        spread = max(spread, abs(a["chi2"][1] - b["chi2"][1]) / max(1.0, a["chi2"][1]))
        gap = max(gap, abs(cases.chi2_at(p, pre, a) - a["chi2"][1]) / max(1.0, a["chi2"][1]))
    print("largest relative chi2 spread between the builds:", spread, "| largest gap to the chi2 at the float outputs:", gap)
    assert spread <= cases.FREE_CHI2_SPREAD and gap <= cases.REEVAL_GAP


X87_FLAGS = ("-O2", "-ffp-contract=off", "-mfpmath=387")   # a third rounding convention: sums and products kept in extended precision


def test_lone_keyframe_turns_on_rounding():
    """The issue's single keyframe with nothing fixed: the oracle's two builds agree on it (they invert the same 3 x 3 blocks, only the
    order of the points differs), yet a build with x87 arithmetic, whose Jacobians round differently, parts from the first by 1e-2 .. 4e-1
    in the states and 5e-4 .. 3e-1 in chi2 on five of the six scenes (the sixth rejects five trials and barely moves) — where a 3-keyframe
    scene parts by 2e-6.  The device's distance from the oracle there (6e-3 .. 1e-1) is of that kind, so these scenes are not compared
    state by state (tests/full_inertial_ba_cases.py, LONE)."""
    try:
        fo.lib(X87_FLAGS)
    except subprocess.CalledProcessError:
        return   # (not an x86 host)
    far = 0
    for c in cases.LONE:
        (p, pre), a = cases.scene(c), cases.case_oracle(c)
        assert p["kfKind"].tolist() == [3]
        b = cases.case_oracle(c, X87_FLAGS)
        d = np.abs(a["kfState"] - b["kfState"]).max()
        print(c[0], "x87 build apart by", d, "chi2", abs(a["chi2"][1] - b["chi2"][1]) / max(a["chi2"][1], 1.0))
        far += d > 1e-3
    assert far >= 4
    c = cases.SMALL[4]
    assert np.abs(cases.case_oracle(c)["kfState"] - cases.case_oracle(c, X87_FLAGS)["kfState"]).max() < 1e-5


def test_corpus_selection():
    """Every case through two builds of the oracle (-O2 -ffp-contract=off, in order; -O3 -ffp-contract=fast, points and links in reverse):
    a case whose stats differ, or whose outputs are more than 1e-6 apart (cases.parting), turns on the rounding of a sum and is no test of
    a kernel; it is listed in LEFT_OUT — at most 3, none of them a tier-edge or a named scene.  The largest relative chi2 spread between
    the builds over the kept cases is pinned: ten times that is the GPU tests' chi2 bound."""
    part = []
    for c in cases.CASES:
        same, d = cases.parting(cases.case_oracle(c), cases.case_oracle(c, fo.OTHER_FLAGS))
        if not same or d > 1e-6:
            part.append(c[0])
    print("cases on which the two builds part:", part)
    assert set(part) <= cases.LEFT_OUT, part
    names = {c[0] for c in cases.CASES}
    assert cases.LEFT_OUT <= names and len(cases.LEFT_OUT) <= 3
    assert not cases.LEFT_OUT & {c[0] for c in cases.TIER + cases.NAMED}
    spread = 0.0
    for c in cases.KEPT:
        a, b = cases.case_oracle(c)["chi2"], cases.case_oracle(c, fo.OTHER_FLAGS)["chi2"]
        spread = max(spread, float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
    print("largest relative chi2 spread between the two builds:", spread)
    assert spread <= cases.CHI2_SPREAD


def test_corpus_covers_the_grid():
    assert len(set(c[0] for c in cases.CASES)) == len(cases.CASES)
    kept = {c[0] for c in cases.KEPT}
    for cam in cases.CAMS:
        for n in (1, 2, 3):
            for b in (0, 1):
                assert f"small-{cam}-{n}kf-init{b}" in kept
    for c in cases.KEPT:
        p, _ = cases.scene(c)
        kw = dict(c[1])
        assert len(p["kfState"]) <= 125 and len(p["mpPos"]) <= 2100 and len(p["eKF"]) <= 15000
        order = np.lexsort((p["eRight"], p["eKF"], p["eMP"]))                   # by point, then keyframe, left before right
        assert (order == np.arange(len(order))).all()
        if kw.get("kb8"):
            r = np.flatnonzero(p["eRight"])
            assert len(r) and (p["eObs"][:, 2] < 0).all()
        elif kw["mono_frac"] == 1.0:
            assert (p["eObs"][:, 2] < 0).all()
        else:
            assert (p["eObs"][:, 2] < 0).any() and (p["eObs"][:, 2] >= 0).any()
        if not kw.get("n_fixed") and not kw.get("observers"):                    # the nothing-fixed gauge: one iteration
            assert not np.isin(p["kfKind"], (1, 2)).any() and c[2] == 1
        linked = np.zeros(len(p["kfKind"]), bool); linked[p["iKF1"]] = True; linked[p["iKF2"]] = True
        assert (np.isin(p["kfKind"], (0, 1)) == linked).all()                     # kinds 0 and 1 are exactly the keyframes of the links
    for c in cases.SMALL:
        p, _ = cases.scene(c)
        n = dict(c[1])["n_kf"]
        assert len(p["iKF1"]) == n - 1 and p["kfKind"].tolist() == ([3, 2] if n == 1 else [0] * n)
    for c in cases.CUT + (cases.GAUGED_CUT,):                                     # kind 3 in the middle, no link across it
        p, _ = cases.scene(c)
        assert p["kfKind"][5] == 3 and not ((p["iKF1"] == 5) | (p["iKF2"] == 5)).any() and (p["eKF"] == 5).any()
        assert (p["iKF1"] < 5).any() and (p["iKF1"] > 5).any()
    for c in cases.SHAPES:                                                        # reach 1: a band of one keyframe; 30: full; loop points: long rows
        (p, _), kw = cases.scene(c), dict(c[1])
        rows, first, count = cases.structure(p)
        per = 3 if kw["init"] else 5
        body = first[:30 * per]
        width = (np.arange(len(body)) - body) // per
        if kw["reach"] == 1:
            assert width.max() == 1
        if kw["reach"] == 30:
            assert np.mean(body == 0) > 0.8
        if kw["n_loop_points"]:
            assert body[-1] == 0 and width[4 * per:-4 * per].max() <= 6
        if kw["init"]:                                                            # the shared row spans everything by construction
            assert len(first) == 30 * per + 2 and (first[-2:] == 0).all()
    its = {c[2] for c in cases.KEPT}
    assert its == {1, 7, 100}


def test_tier_edge_scenes_sit_on_the_constants():
    """One below, on and one above each tier constant of csrc/full_inertial_ba.hip, read off the scenes' own edge and link lists."""
    src = open(os.path.join(ROOT, "morb_slam_amd", "csrc", "full_inertial_ba.hip")).read()
    assert re.search(r"FIBA_NT = 256;", src) and re.search(r"FIBA_ROWS = FIBA_NT / 3;", src) and cases.ROWS_PER_PASS == 256 // 3
    assert re.search(r"FIBA_STAGE = %d;" % cases.LDS_PANEL, src) and re.search(r"FIBA_CHUNK = %d;" % cases.CHUNK, src)
    got = []
    for c in cases.ROWS_EDGE:   # rows covering column 0, the diagonal block's among them
        rows, first, count = cases.structure(cases.scene(c)[0])
        got.append(int((first == 0).sum()))
    assert got == [cases.ROWS_PER_PASS - 1, cases.ROWS_PER_PASS, cases.ROWS_PER_PASS + 1]
    got = []
    for c in cases.PANEL_EDGE:   # blocks of the last row in front of its diagonal block
        rows, first, count = cases.structure(cases.scene(c)[0])
        got.append(int(len(first) - 1 - first[-1]))
    assert got == [cases.LDS_PANEL - 1, cases.LDS_PANEL, cases.LDS_PANEL + 1]
    got = []
    for c in cases.CHUNK_EDGE:
        rows, first, count = cases.structure(cases.scene(c)[0])
        assert len(count) == 6 and len(set(count.values())) == 1
        got.append(count[(1, 0)])
    assert got == [cases.CHUNK - 1, cases.CHUNK, cases.CHUNK + 1] * 2
    for c in cases.CASES:        # and the oracle's own count of unknowns and envelope blocks is the structure's
        rows, first, count = cases.structure(cases.scene(c)[0])
        r = cases.case_oracle(c)
        assert r["stats4"][2] == 3 * len(first) and r["stats4"][3] == int((np.arange(len(first)) - first + 1).sum()), c[0]


def test_named_scenes_do_what_their_names_say():
    for c in cases.NAMED + cases.TIER:
        assert c[0] not in cases.LEFT_OUT
    for c in cases.GAUGED + cases.GAUGED_SMALL + (cases.GAUGED_LARGE, cases.GAUGED_CUT):
        (p, _), r = cases.scene(c), cases.case_oracle(c)
        assert p["kfKind"][0] == 1 and (p["kfKind"][1:] != 1).all()
        assert 1 < r["stats4"][0] <= c[2] and r["chi2"][1] < r["chi2"][0]
        assert r["kfState"][0].tobytes() == p["kfState"][0].tobytes()
    # the 100-iteration scenes end long before they run out: by the stagnation rule, or on the tenth trial of an iteration
    for c in cases.CASES:
        if c[2] == 100:
            r = cases.case_oracle(c)
            assert r["stats4"][0] < 100 and (r["info4"][1] or r["stats4"][1] >= r["stats4"][0] + 9), c[0]
    assert any(not cases.case_oracle(c)["info4"][1] for c in cases.CASES if c[2] == 100)          # (the ten-trials rule does occur)
    assert any(cases.case_oracle(c)["stats4"][1] > cases.case_oracle(c)["stats4"][0] for c in cases.GAUGED_SMALL)      # rejected trials on the way
    for c in (cases.FIXED_PAIR, cases.FIXED_PAIR_INIT):
        (p, _), r = cases.scene(c), cases.case_oracle(c)
        assert p["kfKind"][:3].tolist() == [1, 1, 0] and (p["iKF1"][0], p["iKF2"][0]) == (0, 1)
        assert r["kfState"][:2].tobytes() == p["kfState"][:2].tobytes()
    p, _ = cases.scene(cases.FIXED_PAIR_INIT)
    assert not np.array_equal(cases.case_oracle(cases.FIXED_PAIR_INIT)["bias6"], p["bias6"])
    (p, _), r = cases.scene(cases.OBSERVERS), cases.case_oracle(cases.OBSERVERS)
    assert (p["kfKind"] == 2).sum() == 3 and np.isin(p["eKF"], np.flatnonzero(p["kfKind"] == 2)).any()
    assert r["kfState"][p["kfKind"] == 2].tobytes() == p["kfState"][p["kfKind"] == 2].tobytes()
    (p, _), r = cases.scene(cases.IDLE), cases.case_oracle(cases.IDLE)
    idle = np.setdiff1d(np.arange(len(p["mpPos"])), p["eMP"])
    assert len(idle) == 2 and r["mpPos"][idle].tobytes() == p["mpPos"][idle].tobytes()
    (p, _), r = cases.scene(cases.AT_TRUTH), cases.case_oracle(cases.AT_TRUTH)
    assert np.abs(p["kfState"][:, :15] - p["true"][:, :15]).max() < 1e-6 and r["info4"][3] == 0
    assert r["stats4"][1] > r["stats4"][0] and r["stats4"][0] < 7                       # rejected trials, and the solve ends before it runs out
    for c in (cases.FACTOR_FAILS, cases.FACTOR_FAILS_INIT):                           # ten failed factorisations, nothing moves
        (p, _), r = cases.scene(c), cases.case_oracle(c)
        assert r["stats4"][:2].tolist() == [1, 10] and r["info4"][2] == 1 and np.isfinite(r["chi2"]).all() and r["chi2"][0] == r["chi2"][1]
        assert r["kfState"][:, :15].tobytes() == p["kfState"][:, :15].tobytes() and r["mpPos"].tobytes() == p["mpPos"].tobytes()
        assert r["bias6"].tobytes() == p["bias6"].tobytes()
        if not p["init"]:
            assert r["kfState"].tobytes() == p["kfState"].tobytes()
    # bInit: every kind-0 keyframe ends with the shared biases; without it bias6 is not touched
    for c in (cases.GAUGED[1], cases.SMALL[5]):
        (p, _), r = cases.scene(c), cases.case_oracle(c)
        assert (r["kfState"][p["kfKind"] == 0][:, 15:] == r["bias6"][None, :]).all()
    (p, _), r = cases.scene(cases.GAUGED[0]), cases.case_oracle(cases.GAUGED[0])
    assert r["bias6"].tobytes() == p["bias6"].tobytes()


def test_stop_at_entry_of_the_oracle():
    c = cases.SMALL[5]
    p, pre = cases.scene(c)
    r = fo.run(p, pre, its=c[2], stop_entry=True)
    assert r["stats4"].tolist() == [0] * 4 and r["chi2"].tolist() == [0, 0]
    assert r["kfState"].tobytes() == p["kfState"].tobytes() and r["mpPos"].tobytes() == p["mpPos"].tobytes() and r["bias6"].tobytes() == p["bias6"].tobytes()


def test_header_declares_and_library_exports_the_entries():
    from morb_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_full_inertial_ba\(morb_optimizer\*, int nKF, float\* kfState21, const uint8_t\* kfKind, int nMP, float\* mpPos,", header)
    assert "Optimizer.cc:364-760" in header and "LoopClosing.cc:2305" in header and "LocalMapping.cc:1244-1249" in header
    for name, nargs in (("morb_full_inertial_ba", 29), ("morb_full_inertial_ba_fisheye", 26)):
        restype, argtypes = capi.HEADER.prototypes[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    assert capi.HEADER.prototypes["morb_full_inertial_ba"][1][15:20] == [ctypes.c_float] * 5
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("library not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.lib()
    for name in ("morb_full_inertial_ba", "morb_full_inertial_ba_fisheye"):
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert list(getattr(L, name).argtypes) == capi.HEADER.prototypes[name][1]     # the parsed prototype went through capi.py's loop


def test_kernels_use_no_scratch_memory(tmp_path):
    import test_codeobj_cpu as co
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    if not (os.path.exists(lib) and all(shutil.which(os.path.join(co.LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))):
        pytest.skip("library or LLVM tools not available")
    meta = {k: v for k, v in co._kernel_metadata(lib, str(tmp_path)).items() if re.search(r"\d+k_fiba_\w+?(I|E)", k)}
    assert len(meta) == 13, meta          # twelve kernels, k_fiba_linearize in its pinhole and KannalaBrandt8 forms
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)


def test_reference_typed_member_on_a_mock_map_under_sanitizers(tmp_path):
    """tests/native/full_inertial_ba_member_check.cc: the host-only flattening of FullInertialBA against an edge and link list written by hand
    (a bad keyframe, a keyframe without IMU, a keyframe past maxKFid, a missing mPrevKF, a rig keyframe with left and right observations,
    bFixLocal with 2 and with 3 free keyframes), both write-backs, the shared-bias write-back, the handle per caller, a raised stop flag, and
    the three call-site lines of LoopClosing.cc:2305 and LocalMapping.cc:1244-1249 verbatim, with the C entries stubbed in the program; built
    with -fsanitize=address,undefined as a stand-alone program."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "full_inertial_ba_member_check")
    src_path = os.path.join(native, "full_inertial_ba_member_check.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(native, "mock_full_inertial_ba"), "-I" + os.path.join(native, "mock_ref"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe, src_path])
    src = open(src_path).read()
    assert "    Optimizer::FullInertialBA(pActiveMap, 7, false, nLoopKF, &mbStopGBA);\n" in src
    assert ("    Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false,\n                              mpCurrentKeyFrame->mnId, NULL, true, priorG,\n"
            "                              priorA);\n") in src
    assert "    Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false,\n                              mpCurrentKeyFrame->mnId, NULL, false);\n" in src
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "full inertial ba member ok" in out.stdout, out.stdout + out.stderr
