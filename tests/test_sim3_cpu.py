"""Optimizer::OptimizeSim3: the CPU oracle (tests/native/sim3_oracle.cc) on problems with a known answer, the exp(+-1e-9) constants of
the kernel against the host libm, and the C ABI entry point in the library's header."""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest

import sim3_oracle
from morb_slam_amd.synth import make_sim3_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exact_problem(n=60, scale=2.0, seed=0):
    """Noise-free correspondences whose every intermediate value is exact in float: identity keyframe poses, dyadic points and pixel
    parameters, S12 = (180 degrees about z, dyadic t, power-of-two scale).  The true S12 is then a zero of every residual."""
    rng = np.random.default_rng(seed)
    cam = np.array([0, 256, 256, 320, 240, 0, 0, 0, 0], np.float32)
    z1 = 2.0 ** rng.integers(1, 4, n)
    X1 = np.stack([rng.integers(-64, 64, n) / 128 * z1, rng.integers(-48, 48, n) / 128 * z1, z1], 1)
    q = np.array([0, 0, 1.0, 0]); t = np.array([0.25, -0.5, 0.0])
    X2 = np.stack([-(X1[:, 0] - t[0]) / scale, -(X1[:, 1] - t[1]) / scale, X1[:, 2] / scale], 1)
    proj = lambda X: np.stack([256 * X[:, 0] / X[:, 2] + 320, 256 * X[:, 1] / X[:, 2] + 240], 1)
    T = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    S_true = np.concatenate([q, t, [scale]])
    S0 = S_true.copy()
    S0[:4] = np.array([0.004, -0.003, 0.99998, 0.002]) / np.linalg.norm([0.004, -0.003, 0.99998, 0.002])
    S0[4:7] += [0.01, -0.02, 0.015]
    S0[7] *= 1.0 if scale == 1.0 else 1.03
    return dict(n=n, entry=np.full(n, 3, np.uint8), Xw1=X1.astype(np.float32), Xw2=X2.astype(np.float32),
                i2=np.arange(n, dtype=np.int32), obs1=proj(X1).astype(np.float32), inv1=np.ones(n, np.float32),
                obs2=proj(X2).astype(np.float32), inv2=np.ones(n, np.float32), T1w=T, T2w=T.copy(), cam1=cam, cam2=cam.copy(),
                th2=np.float32(10.0), fix_scale=scale == 1.0, S12=S0, S12_true=S_true)


def _same_rotation(qa, qb):
    return min(np.abs(qa - qb).max(), np.abs(qa + qb).max())


@pytest.mark.parametrize("scale", [2.0, 1.0])
def test_oracle_recovers_known_sim3(scale):
    p = _exact_problem(scale=scale)
    nIn, keep, S, st = sim3_oracle.solve(p)
    assert nIn == p["n"] and keep.all() and st[4] == 1
    assert np.abs(np.linalg.norm(S[:4]) - 1) <= 1e-9
    assert _same_rotation(S[:4] / np.linalg.norm(S[:4]), p["S12_true"][:4]) <= 1e-9
    assert np.abs(S[4:] - p["S12_true"][4:]).max() <= 1e-9
    if scale == 1.0:
        assert S[7] == 1.0          # bFixScale: the scale never moves


def _correspondences(p):
    e = p["entry"]
    return (e & 1).astype(bool) & (e & 2).astype(bool) & ~(e & 4).astype(bool) & ~(e & 8).astype(bool) & ((p["i2"] >= 0))


@pytest.mark.parametrize("fix", [False, True])
def test_oracle_nulls_planted_outliers(fix):
    p = make_sim3_problem(400, seed=7, fix_scale=fix, outlier_frac=0.25, bad_frac=0.05, no_mp1_frac=0.05, noise_px=0.3)
    nIn, keep, S, st = sim3_oracle.solve(p)
    corr = _correspondences(p)
    planted = p["outlier"] & corr
    assert planted.sum() > 50 and st[4] == 1
    assert (keep[planted] == 0).all()
    assert keep[corr & ~p["outlier"]].mean() > 0.97
    assert nIn == int(keep[corr].sum())
    assert _same_rotation(S[:4], p["S12_true"][:4]) < 1e-3 and abs(S[7] - p["S12_true"][7]) < 1e-3
    # entries that are not correspondences keep their match
    assert (keep[~corr] == (p["entry"][~corr] & 1)).all()


def test_oracle_early_return_leaves_s12():
    p = make_sim3_problem(40, seed=3, outlier_frac=0.0, unmatched_frac=0.0)
    p["entry"][12:] = 0                      # 12 correspondences ...
    p["obs1"][:5] += 80.0                     # ... 5 of them gross outliers: 7 survivors < 10
    S0 = p["S12"].copy()
    nIn, keep, S, st = sim3_oracle.solve(p)
    assert nIn == 0 and st[4] == 0 and st[5] == 12 and st[6] >= 3
    assert S.tobytes() == S0.tobytes()
    assert (keep[:5] == 0).all()              # the phase-1 nulls stay


def test_oracle_zero_correspondences():
    p = make_sim3_problem(30, seed=4)
    p["entry"][:] = p["entry"] & ~np.uint8(2)   # no pMP1 anywhere
    S0 = p["S12"].copy()
    nIn, keep, S, st = sim3_oracle.solve(p)
    assert nIn == 0 and st[4] == 0 and st[5] == 0 and st[0] == 0
    assert S.tobytes() == S0.tobytes() and (keep == (p["entry"] & 1)).all()
    q = make_sim3_problem(1, seed=5)
    q["n"] = 0
    assert sim3_oracle.solve(q)[0] == 0


def test_exp_constants_match_host_libm():
    src = open(os.path.join(ROOT, "morb_slam_amd", "csrc", "sim3.hip")).read()
    consts = dict(re.findall(r"S3_EXP_([PM]) = (0x[0-9a-fA-Fp.+-]+);", src))
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.exp.restype = C.c_double
    libm.exp.argtypes = [C.c_double]
    assert float.fromhex(consts["P"]) == libm.exp(1e-9)
    assert float.fromhex(consts["M"]) == libm.exp(-1e-9)


def test_header_declares_sim3_entry():
    h = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    assert re.search(r"int morb_optimize_sim3_batch\(morb_optimizer\*", h)


def test_reference_signature_member_compiles():
    """tests/native/sim3_call_check.cc calls Optimizer::OptimizeSim3 in the reference's call form against mock keyframes / map points / g2o::Sim3;
    compiled to an object, the member template must be instantiated."""
    import subprocess
    import tempfile
    nat = os.path.join(ROOT, "tests", "native")
    with tempfile.TemporaryDirectory() as td:
        obj = os.path.join(td, "sim3_call.o")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-o", obj, "-I" + os.path.join(nat, "mock_ref"), "-I" + os.path.join(nat, "mock_sim3"),
                            "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                            os.path.join(nat, "sim3_call_check.cc")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        syms = subprocess.run(["nm", "-C", obj], capture_output=True, text=True, check=True).stdout
    assert "Optimizer::OptimizeSim3<ORB_SLAM3::KeyFrame, ORB_SLAM3::MapPoint, g2o::Sim3, Eigen::Matrix<double, 7, 7> >" in syms or \
        "Optimizer::OptimizeSim3<ORB_SLAM3::KeyFrame, ORB_SLAM3::MapPoint, g2o::Sim3, Eigen::Matrix<double, 7, 7>>" in syms


def test_libm_f64_matches_host_libm():
    """csrc/libm_f64.h (glibc 2.35's double sin / cos / exp as its FMA build runs them: the cos / sin of KannalaBrandt8::project and of the Sim3
    exponential on the device) against the host libm, bit for bit, over float-valued angles in [-pi, pi] (KB8's psi) and general arguments."""
    import subprocess
    import tempfile
    flags = open("/proc/cpuinfo").read()
    assert " fma " in flags and " avx2 " in flags, "the reference libm restated here is glibc's FMA / AVX2 variant"
    src = r'''
#include <cmath>
#include <cstdio>
#include <random>
#include "libm_f64.h"
int main() {
  std::mt19937_64 g(11); std::uniform_real_distribution<float> u(-3.1415927f, 3.1415927f); std::uniform_real_distribution<double> w(-40.0, 40.0);
  long bad = 0;
  for (long i = 0; i < 3000000; ++i) {
    const double x = (i % 3 == 0) ? (double)u(g) : (i % 3 == 1) ? w(g) : std::ldexp(w(g), -(int)(i % 60));
    if (morbm64::sin_glibc(x) != std::sin(x) || morbm64::cos_glibc(x) != std::cos(x)) { if (bad < 5) printf("%a\n", x); ++bad; }
    double s, c;
    morbm64::sincos_glibc(x, &s, &c);
    double hs, hc;
    sincos(x, &hs, &hc);
    if (s != hs || c != hc) { if (bad < 5) printf("sincos %a\n", x); ++bad; }
    const double y = std::ldexp(w(g), -(int)(i % 50));   // the scale component of an LM step
    if (morbm64::exp_glibc(y) != std::exp(y)) { if (bad < 5) printf("exp %a\n", y); ++bad; }
  }
  printf("mismatches %ld\n", bad);
  return bad != 0;
}
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "chk.cc")
        open(c, "w").write(src)
        exe = os.path.join(td, "chk")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "morb_slam_amd", "csrc"), "-o", exe, c])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
