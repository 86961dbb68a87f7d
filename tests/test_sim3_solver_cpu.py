"""Sim3Solver: the CPU oracle (tests/native/sim3_solver_oracle.cc) on problems with a known answer, the scalar pieces the kernel shares
with the adapter (include/morb/sim3_solver_math.h: RANSAC budget, truncated thresholds, the double atan2) against the host, the new kernel's
scratch use, and the C++ adapter against mock reference types."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sim3_solver_oracle
from morb_slam_amd.synth import libc_rand, make_sim3_solver_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def ssm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ssm") / "libssm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(NATIVE, "sim3_solver_math_check.cc")])
    L = C.CDLL(out)
    L.ssm_budget.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int]
    L.ssm_budget_ratio.argtypes = [C.c_int, C.c_int, C.c_double]
    L.ssm_budget_ratio.restype = C.c_double
    L.ssm_max_error.argtypes = [C.c_float]
    L.ssm_max_error.restype = C.c_float
    L.ssm_random_int.argtypes = [C.c_int, C.c_int]
    L.ssm_atan2_check.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("cams", [("pinhole", "pinhole"), ("kb8", "kb8"), ("pinhole", "kb8")])
@pytest.mark.parametrize("fix", [False, True])
def test_oracle_recovers_known_sim3(cams, fix):
    p = make_sim3_solver_problem(300, seed=3, cam1=cams[0], cam2=cams[1], fix_scale=fix, outlier_frac=0.0, noise_px=0.0, dup_frac=0.0,
                                 bad_frac=0.0, no_mp1_frac=0.0, neg_idx_frac=0.0, unmatched_frac=0.0)
    calls, best = sim3_solver_oracle.run(p, libc_rand(11, 900))
    c = calls[-1]
    assert c["converged"] == 1 and c["nInliers"] == c["N"] == 300 and c["iterations"] == 1 and c["mask"].all()
    S = p["S12_true"]
    T = best["bestT12"].reshape(4, 4)
    assert np.abs(best["bestR"].reshape(3, 3) - _rot(S[:4])).max() <= 1e-5
    assert abs(best["bestScale"] - S[7]) <= 1e-5 * S[7]
    assert np.abs(T[:3, :3] - best["bestScale"] * best["bestR"].reshape(3, 3)).max() <= 1e-6
    assert np.abs(best["bestt"] - S[4:7]).max() <= 1e-5
    assert np.array_equal(c["sim3"], best["bestT12"])
    if fix:
        assert best["bestScale"] == 1.0


def test_oracle_chunked_equals_one_call():
    p = make_sim3_solver_problem(400, seed=5, outlier_frac=0.75, min_inliers=30)
    r = libc_rand(21, 900)
    one, b1 = sim3_solver_oracle.run(p, r)
    chunks, b2 = sim3_solver_oracle.run(p, r, calls=[20] * 15)
    assert one[-1]["iterations"] == chunks[-1]["iterations"] > 20
    assert np.array_equal(b1["hyp"], b2["hyp"]) and np.array_equal(b1["bestT12"], b2["bestT12"])
    assert one[-1]["converged"] == chunks[-1]["converged"] and np.array_equal(one[-1]["mask"], chunks[-1]["mask"])


def test_max_error_is_the_truncated_size_t(ssm):
    # mvnMaxError1 / 2 are std::vector<size_t>: 9.210 * sigma2 loses its fraction, then compares as a float
    lev = ((1.2 ** np.arange(8)) ** 2).astype(np.float32)
    got = [ssm.ssm_max_error(float(s)) for s in lev]
    assert got == [float(int(9.210 * float(s))) for s in lev]
    assert got[:4] == [9.0, 13.0, 19.0, 27.0]   # not 9.21, 13.26, 19.10, 27.50
    # the oracle applies it: a correspondence whose reprojection error is ~9.1 px^2 on both sides (inside [9, 9.21)) is an outlier at
    # octave 0 (threshold 9, not 9.21) and an inlier at octave 1 (threshold 13)
    p = _threshold_problem()
    d = p["displaced"]
    f32 = np.float32
    R1, t1, c1 = p["T1w"][:9].reshape(3, 3), p["T1w"][9:], p["cam1"]
    X = lambda Xw: np.array([R1[r, 0] * Xw[0] + R1[r, 1] * Xw[1] + R1[r, 2] * Xw[2] + t1[r] for r in range(3)], np.float32)
    uv = lambda Xc: np.array([c1[1] * Xc[0] / Xc[2] + c1[3], c1[2] * Xc[1] / Xc[2] + c1[4]], np.float32)
    q = make_sim3_solver_problem(p["n"], seed=21, outlier_frac=0.0, noise_px=0.0, dup_frac=0.0, bad_frac=0.0, no_mp1_frac=0.0,
                                 neg_idx_frac=0.0, unmatched_frac=0.0, min_inliers=10)
    err = float(((uv(X(p["Xw1"][d])) - uv(X(q["Xw1"][d]))) ** 2).sum())   # vs where the true Sim3 maps pMP2: the undisplaced pMP1
    assert 9.05 < err < 9.16, err
    calls, _ = sim3_solver_oracle.run(p, libc_rand(1, 900))
    c = calls[-1]
    assert c["converged"] and c["N"] == p["n"] and c["nInliers"] == p["n"] - 1, (c["nInliers"], np.nonzero(c["mask"] == 0)[0])
    assert c["mask"][d] == 0 and c["mask"].sum() == p["n"] - 1
    p["sigma2_1"][d] = LEV1
    calls, _ = sim3_solver_oracle.run(p, libc_rand(1, 900))
    assert calls[-1]["converged"] and calls[-1]["nInliers"] == p["n"] and calls[-1]["mask"][d] == 1


LEV1 = np.float32(1.44)
LEV7 = np.float32(1.2 ** 14)


def _threshold_problem(n=150, d=7):
    """make_sim3_solver_problem's noise-free geometry (a real Sim3 between the keyframes) with feature d's pMP1 moved along KF1's camera
    x axis by sqrt(9.1) px at its depth; side 2 of d gets a wide threshold (octave 7), so side 1 decides."""
    p = make_sim3_solver_problem(n, seed=21, outlier_frac=0.0, noise_px=0.0, dup_frac=0.0, bad_frac=0.0, no_mp1_frac=0.0, neg_idx_frac=0.0,
                                 unmatched_frac=0.0, min_inliers=10)
    p["sigma2_1"][:] = 1.0
    p["sigma2_2"][:] = 1.0
    p["sigma2_2"][d] = LEV7
    R1, t1 = p["T1w"][:9].reshape(3, 3).astype(np.float64), p["T1w"][9:].astype(np.float64)
    z = (R1 @ p["Xw1"][d] + t1)[2]
    p["Xw1"] = p["Xw1"].copy()
    p["Xw1"][d] = (p["Xw1"][d] + R1.T @ np.array([np.sqrt(9.1) * z / p["cam1"][1], 0, 0])).astype(np.float32)
    p["displaced"] = d
    return p


def test_budget_matches_the_host_formula_exhaustively(ssm):
    for m in (6, 15, 20, 30):
        for N in range(0, 8193):
            assert ssm.ssm_budget(N, m, 0.99, 300) == sim3_solver_oracle.budget(N, m, 0.99, 300), (N, m)
    # the x86 conversion of an out-of-range ceil: minInliers / N below ~1.29e-3 gives a budget of 1 in the reference
    assert sim3_solver_oracle.budget(8192, 6, 0.99, 300) == 1 and ssm.ssm_budget(8192, 6, 0.99, 300) == 1
    assert sim3_solver_oracle.budget(400, 20, 0.99, 300) == 300 and sim3_solver_oracle.budget(40, 20, 0.99, 300) == 35


def test_budget_does_not_hang_on_the_last_bits_of_log_and_pow(ssm):
    # the device evaluates log / pow with its own library (a few ulp from glibc's).  The budget is min(ceil(ratio), maxIterations),
    # so only ratios up to maxIterations (here up to 10^4) and the int overflow at 2^31 can feel that: for every N <= 8192 and the
    # minInliers in use, those ratios stay clear of an integer by 1e-9 (relative) and of 2^31 by 1e-5
    for m in (6, 15, 20, 30):
        for N in range(m + 1, 8193):
            x = ssm.ssm_budget_ratio(N, m, 0.99)
            if x < 1e4:
                assert x != np.round(x) and abs(x - np.round(x)) > 1e-9 * x, (N, m, x)
            assert abs(x - 2.0 ** 31) > 1e-5 * x, (N, m, x)


def _two_view_sampling_pairs():
    """The (rand() value, size) pairs of tests/native/two_view_math_check.cc: its sizes, its xorshift stream, eight draws per set."""
    s, N, pairs = 88172645463325252, 8, []
    while N <= 2000:
        for rep in range(200):
            for j in range(8):
                if rep < 2:
                    r = 0 if rep == 0 else 2 ** 31 - 1
                else:
                    s ^= (s << 13) & (2 ** 64 - 1)
                    s ^= s >> 7
                    s ^= (s << 17) & (2 ** 64 - 1)
                    r = s >> 33
                pairs.append((r, N - j))
        N = N + 1 if N < 40 else N * 3 // 2
    return pairs


def test_random_int_matches_dutils(ssm):
    """morbransac::random_int (include/morb/ransac_math.h), the one RandomInt of the three solvers, against the reference's double
    expression: the inputs each solver's own check used (Sim3Solver's, MLPnPsolver's, the sampling sets of TwoViewReconstruction)."""
    rng = np.random.default_rng(0)
    pairs = list(zip(rng.integers(0, 2 ** 31, 20000), rng.integers(1, 8193, 20000))) + [(2 ** 31 - 1, 8192), (0, 1), (2 ** 31 - 1, 1)]
    rng = np.random.default_rng(0)
    pairs += list(zip(rng.integers(0, 2 ** 31, 5000), rng.integers(1, 4097, 5000))) + [(2 ** 31 - 1, 4096), (0, 1)]
    pairs += _two_view_sampling_pairs()
    assert len(pairs) > 90000
    for r, d in pairs:
        assert ssm.ssm_random_int(int(r), int(d)) == int((float(r) / (2147483647 + 1.0)) * int(d))


def test_atan2_restatement_matches_host_libm(ssm):
    rng = np.random.default_rng(1)
    n = 1 << 21
    # ComputeSim3's arguments: y = |imaginary part| in [0, 1], x = real part in [-1, 1] of a unit float quaternion; plus general floats
    y = np.concatenate([rng.random(n), np.abs(rng.normal(0, 1e-4, n)), np.abs(rng.standard_cauchy(n)),
                        [0, 0, 1, 1, 0, np.inf, np.nan, 1e-30, 1e30]]).astype(np.float32)
    x = np.concatenate([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.standard_cauchy(n),
                        [1, -1, 0, -0.0, 0, 1, 1, -1e30, -1e-30]]).astype(np.float32)
    q = rng.normal(0, 1, (n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    y = np.concatenate([y, np.sqrt((q[:, 1:] ** 2).sum(1))]).astype(np.float32)
    x = np.concatenate([x, q[:, 0]]).astype(np.float32)
    a, b = C.c_int(-1), C.c_int(-1)
    ssm.ssm_atan2_check(len(x), y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b))
    assert a.value == 0, f"{a.value} of {len(x)} differ after (float)(2 * atan2)"


def _kernel_scratch(lib, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    meta = {}
    for i, st in enumerate(starts):
        en = starts[i + 1] if i + 1 < len(starts) else len(blob)
        bun, co = os.path.join(tmp, f"bundle{i}.bin"), os.path.join(tmp, f"code{i}.o")
        open(bun, "wb").write(blob[st:en])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + bun, "--output=" + co])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", notes, re.S):
            meta[m.group(1)] = int(m.group(2))
    return meta


def test_sim3_solver_kernel_uses_no_scratch(tmp_path):
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    assert os.path.exists(lib), "build() first"
    assert all(shutil.which(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    meta = _kernel_scratch(lib, str(tmp_path))
    ks = {k: v for k, v in meta.items() if "k_sim3_solver" in k and not k.endswith(".kd")}
    assert ks, "k_sim3_solver is missing from the library"
    assert all(v == 0 for v in ks.values()), ks


def test_reference_call_form_compiles_against_mocks(tmp_path):
    """tests/native/sim3_solver_call_check.cc pastes LoopClosing.cc:700-722 verbatim against mock keyframes / map points / Matrix4f
    (tests/native/mock_sim3_solver); compiled to an object, the adapter's constructor template and members must be instantiated."""
    obj = str(tmp_path / "ss_call.o")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-o", obj, "-I" + os.path.join(NATIVE, "mock_ref"),
                        "-I" + os.path.join(NATIVE, "mock_sim3_solver"), "-I" + os.path.join(ROOT, "include", "morb"),
                        "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", os.path.join(NATIVE, "sim3_solver_call_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", obj], capture_output=True, text=True, check=True).stdout
    assert re.search(r"Sim3Solver::Sim3Solver<ORB_SLAM3::KeyFrame, ORB_SLAM3::MapPoint>", syms)
    assert "ORB_SLAM3::Sim3Solver::run(" in syms or "Sim3Solver::iterate(" in syms
