"""TwoViewReconstruction without a GPU: the CPU oracle (tests/native/two_view_oracle.cc) and what the kernel shares with it.
The oracle's null-vector and SVD routines against numpy, its poses against the ground truth of the successful corpus problems, the
sampling against a transcription of the reference's loop, the corpus through the oracle built three ways, acosf of csrc/libm_f32.h
against this machine's libm over every float of [-1, 1], the d_stats / d_fstats enums against the Python front's tuples, the
library's export, the kernel's scratch use, the C++ adapter against mock reference types, and include/morb/two_view_math.h under
sanitizers in a stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import two_view_corpus
import two_view_oracle
from morb_slam_amd.optimizer import TWO_VIEW_FAIL, TWO_VIEW_FSTATS, TWO_VIEW_STATS
from morb_slam_amd.synth import libc_rand
from test_sim3_solver_cpu import _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LLVM = "/opt/rocm/lib/llvm/bin"
FAST = ("-O3", "-ffp-contract=fast", "-march=native")
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


@pytest.fixture(scope="module")
def corpus():
    probs, rands = two_view_corpus.problems()
    return probs, rands, [two_view_oracle.run(p, r) for p, r in zip(probs, rands)]


def test_null_vector_and_svd_against_numpy():
    """The routines that stand in for Eigen's JacobiSVD.  A float input is exact in FP64; A^T A is formed and solved in FP64, so the
    null vector carries an error of about eps64 * cond(A)^2 relative to the gap, and is then rounded to float: the bound is
    4 * eps32 + 64 * eps64 * (s_max / s_gap)^2 on the sine of the angle to numpy's vector, with s_gap the second smallest singular
    value (the smallest is 0 for 8 x 9 and about noise for 16 x 9).  Singular values of a 3 x 3: sqrt of an FP64 eigenvalue of M^T M,
    absolute error eps64 * s_max^2 / s, rounded to float: 4 * eps32 * s_max + 64 * eps64 * s_max^2 / s."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for rows, m in ((8, 9), (16, 9), (4, 4)):
        for _ in range(40):
            A = rng.normal(0, 1, (rows, m)).astype(np.float32)
            if rows >= m:   # make the last singular value small, as a 16 x 9 homography system or a 4 x 4 triangulation has it
                u, s, vt = np.linalg.svd(A.astype(np.float64), full_matrices=False)
                s[-1] = s[-2] * 1e-3
                A = ((u * s) @ vt).astype(np.float32)
            x = two_view_oracle.null_vector(A).astype(np.float64)
            _, s, vt = np.linalg.svd(A.astype(np.float64))
            s_gap = s[m - 2]
            sine = float(np.linalg.norm(x / np.linalg.norm(x) - vt[-1] * np.sign(vt[-1] @ x)))
            bound = 4 * EPS32 + 64 * EPS64 * (s[0] / s_gap) ** 2
            worst = max(worst, sine / bound)
            assert abs(np.linalg.norm(x) - 1) <= 4 * EPS32 and sine <= bound, (rows, m, sine, bound)
    for _ in range(60):
        M = rng.normal(0, 1, (3, 3)).astype(np.float32)
        U, w, V = (a.astype(np.float64) for a in two_view_oracle.svd3(M))
        s = np.linalg.svd(M.astype(np.float64), compute_uv=False)
        tol = 4 * EPS32 * s[0] + 64 * EPS64 * s[0] ** 2 / s
        assert (np.abs(np.abs(w) - s) <= tol).all() and (w[:2] >= 0).all(), (w, s, tol)
        assert np.abs(U.T @ U - np.eye(3)).max() <= 8 * EPS32 and np.abs(V.T @ V - np.eye(3)).max() <= 8 * EPS32
        assert abs(np.linalg.det(U) - 1) <= 16 * EPS32 and abs(np.linalg.det(V) - 1) <= 16 * EPS32   # u2 = u0 x u1, v2 = v0 x v1
        assert (w[2] < 0) == (np.linalg.det(M.astype(np.float64)) < 0)
        rec = (U * w) @ V.T
        assert np.abs(rec - M).max() <= 16 * EPS32 * s[0] + 64 * EPS64 * s[0] ** 2 / s[2], np.abs(rec - M).max()
    print(f"null vector: largest sine / bound {worst:.3f}")
    E = np.array([[0, -0.3, 0.1], [0.3, 0, -0.9], [-0.1, 0.9, 0]], np.float32)   # an essential matrix: singular values (s, s, 0)
    U, w, V = two_view_oracle.svd3(E)
    assert abs(w[2]) <= 1e-6 and abs(w[0] - w[1]) <= 1e-6 and np.abs(U[:, 2] @ E.astype(np.float64)).max() <= 1e-6


def test_oracle_recovers_the_ground_truth(corpus):
    """Successful problems against the scene's T21.  Bound: the pixel noise n over the focal length f is an angular noise n / f per
    ray; a rotation fitted to N rays with a conditioning loss of up to 10 (the translation takes most of the parallax signal with it)
    errs by about 10 n / (f sqrt(N)), the translation direction by that over the parallax angle (baseline / depth ~ 0.08).  With
    n <= 1 px, f = 520, N >= 100 that is 0.11 and 1.4 degrees; the bounds are 1 and 8 degrees (about 8 and 6 sigma), and 1.5 / 8 for
    the corner scenes, whose five distinct points determine H with no redundancy to average over."""
    probs, _, oracle = corpus
    n = 0
    for k, (p, o) in enumerate(zip(probs, oracle)):
        if not o["ok"]:
            continue
        R, t = o["T21"][:9].reshape(3, 3).astype(np.float64), o["T21"][9:].astype(np.float64)
        Rt, tt = p["T21_true"][:3, :3], p["T21_true"][:3, 3]
        rot = float(np.degrees(np.arccos(np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1))))
        tdir = float(np.degrees(np.arccos(np.clip(t @ tt / (np.linalg.norm(t) * np.linalg.norm(tt)), -1, 1))))
        print(f"problem {k} ({p['kind']}, model {o['MODEL']}): rotation {rot:.3f} deg, translation direction {tdir:.3f} deg")
        assert abs(np.linalg.norm(t) - 1) <= 1e-5 and abs(np.linalg.det(R) - 1) <= 1e-4
        assert rot <= (1.5 if p["kind"] == "corners" else 1.0) and tdir <= 8.0, (k, rot, tdir)
        tri = o["triangulated"].astype(bool)
        assert tri.sum() >= 50 and (o["P3D"][tri, 2] > 0).all()
        n += 1
    assert n >= 9
    two_view_corpus.assert_composition(probs, oracle)


def test_sampling_equals_the_reference_loop():
    for N, its, seed in ((8, 50, 1), (9, 50, 2), (150, 200, 3), (1500, 200, 4)):
        r = libc_rand(seed, 8 * its)
        want = np.zeros((its, 8), np.int32)
        k = 0
        for it in range(its):                      # :82-95
            avail = list(range(N))
            for j in range(8):
                randi = int((float(r[k]) / (2147483647 + 1.0)) * ((len(avail) - 1) - 0 + 1)) + 0
                k += 1
                want[it, j] = avail[randi]
                avail[randi] = avail[-1]
                avail.pop()
        assert np.array_equal(two_view_oracle.sets(N, its, r), want), N
        assert all(len(set(row)) == 8 for row in want)


def _same(a, b, k, exact):
    for f in ("ok",) + TWO_VIEW_STATS:
        assert a[f] == b[f], (k, f, a[f], b[f])
    assert np.array_equal(a["inliersH"], b["inliersH"]) and np.array_equal(a["inliersF"], b["inliersF"]), k
    assert np.array_equal(a["triangulated"], b["triangulated"]), k
    if exact:
        for f in ("T21", "P3D", "fstats", "hyp"):
            assert a[f].tobytes() == b[f].tobytes(), (k, f)
    else:
        assert np.abs(a["T21"] - b["T21"]).max() <= 1e-4, k


def test_optimisation_level_does_not_change_a_bit(corpus):
    probs, rands, oracle = corpus
    for k, (p, r) in enumerate(zip(probs, rands)):
        _same(oracle[k], two_view_oracle.run(p, r, flags=("-O0", "-ffp-contract=off")), k, exact=True)


def test_rounding_does_not_move_the_corpus(corpus):
    """ok, the model, every count, both masks and vbTriangulated are the same with contraction allowed (-O3 -ffp-contract=fast
    -march=native): the exact comparison on the GPU judges the kernel, not rounding.  A seed that fails here is replaced in
    tests/two_view_corpus.py, never tolerated."""
    probs, rands, oracle = corpus
    for k, (p, r) in enumerate(zip(probs, rands)):
        _same(oracle[k], two_view_oracle.run(p, r, flags=FAST), k, exact=False)


def test_acosf_restatement_matches_this_libm(tmp_path):
    """csrc/libm_f32.h's acosf_glibc against this machine's acosf over EVERY float in [-1, 1] (both signs, zeros and denormals) and
    a sample of NaNs, infinities and |x| > 1 (NaN on both sides)."""
    src, exe = tmp_path / "acosf_check.cc", tmp_path / "acosf_check"
    src.write_text(r'''
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>
#include <atomic>
#include "libm_f32.h"
int main() {
  std::atomic<long> bad{0}, n{0};
  auto same = [](float a, float b) { return (a != a && b != b) || morbm::f2u(a) == morbm::f2u(b); };
  std::vector<std::thread> th;
  for (int w = 0; w < 8; ++w) th.emplace_back([&, w] {
    long nn = 0;
    for (uint64_t u = w; u < (1ull << 32); u += 8) {
      const uint32_t ix = (uint32_t)u & 0x7fffffffu;
      if (ix > 0x3f800000u && ((uint32_t)u & 0x3ffu) != 0x155u && ix != 0x7f800000u) continue;   // beyond [-1, 1]: one in 1024, and +-inf
      const float x = morbm::u2f((uint32_t)u);
      ++nn;
      if (!same(morbm::acosf_glibc(x), acosf(x))) { if (bad++ < 5) printf("acosf(%a) = %a, libm %a\n", x, morbm::acosf_glibc(x), acosf(x)); }
    }
    n += nn;
  });
  for (auto& t : th) t.join();
  printf("checked %ld mismatches %ld\n", n.load(), bad.load());
  return bad != 0;
}
''')
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "morb_slam_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-500:]
    assert int(out.stdout.split()[1]) >= 2 * 0x3f800000   # every float of [-1, 1]


def test_math_header_under_sanitizers_and_enum_names(tmp_path):
    """tests/native/two_view_math_check.cc, a program of its own, with -fsanitize=address,undefined: tv_sample8 against the vector
    form, the scalar pieces, and the enums by name, which must be the Python front's tuples in order."""
    exe = str(tmp_path / "two_view_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "two_view_math_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    lines = out.stdout.splitlines()
    stats = [ln.split()[1:] for ln in lines if ln.startswith("stat ")]
    fstats = [ln.split()[1:] for ln in lines if ln.startswith("fstat ")]
    assert [n for n, _ in stats] == list(TWO_VIEW_STATS) and [int(v) for _, v in stats] == list(range(len(TWO_VIEW_STATS)))
    assert [n for n, _ in fstats] == list(TWO_VIEW_FSTATS) and [int(v) for _, v in fstats] == list(range(len(TWO_VIEW_FSTATS)))
    assert f"len {len(TWO_VIEW_STATS)} {len(TWO_VIEW_FSTATS)}" in lines
    assert "fail " + " ".join(str(k) for k in range(len(TWO_VIEW_FAIL))) in lines


def test_library_exports_the_entry_and_the_kernel_uses_no_scratch(tmp_path):
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    assert os.path.exists(lib), "build() first"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT morb_two_view_reconstruction_batch\b", nm)
    assert all(shutil.which(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    meta = _kernel_scratch(lib, str(tmp_path))
    ks = {k: v for k, v in meta.items() if "k_two_view" in k and not k.endswith(".kd")}
    assert ks, "k_two_view is missing from the library"
    assert all(v == 0 for v in ks.values()), ks


def test_python_front_and_synth_are_there():
    from morb_slam_amd import Optimizer
    from morb_slam_amd import synth
    assert callable(Optimizer.TwoViewReconstruction) and callable(synth.pack_two_view_problems)
    for kind in synth.TWO_VIEW_KINDS:
        p = synth.make_two_view_problem(3, kind, n1=90, n2=80, n_matches=40)
        assert (p["matches12"] >= 0).sum() == 40 and p["kp1"].shape == (90, 2) and p["kp2"].shape == (80, 2)
        assert len(set(p["matches12"][p["matches12"] >= 0])) == 40 and p["matches12"].max() < 80


def test_adapter_and_call_site_compile_against_mocks():
    """include/morb/TwoViewReconstruction.h and a Pinhole::ReconstructWithTwoViews written against the mocks of tests/native/mock_ref and
    tests/native/mock_two_view (tests/native/two_view_call_check.cc): -fsyntax-only."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(NATIVE, "mock_ref"),
                        "-I" + os.path.join(NATIVE, "mock_two_view"), "-I" + os.path.join(ROOT, "include", "morb"),
                        "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", os.path.join(NATIVE, "two_view_call_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
