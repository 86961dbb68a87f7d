"""What the device-math tests (test_device_math_gpu.py) stand on, checked without a GPU:
  * the host entries of tests/native/libmath_probe.so return this machine's libm's bits — the same pin tests/test_oracle_cpu.py,
    test_two_view_cpu.py and test_sim3_cpu.py hold the g++ build of the headers to, here for the probe's own host build;
  * the Python model of the DPP scan of csrc/wave.h agrees with a per-lane simulation of its six steps;
  * every branch the GPU tests are to enter has its 100 inputs;
  * the bounds of math_probe.py (BOUNDS, C_JACOBI, C_CLAMP, C_INVERT) are what the FP64 transcriptions measure against mpmath / eigh."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

import math_probe as P

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")


def _libm_f32(name, *cols):
    f = getattr(_libm, name)
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * len(cols)
    return np.array([f(*[float(c) for c in row]) for row in zip(*cols)], np.float32)


@pytest.mark.parametrize("name", ["atanf", "acosf", "tanf", "sinf", "cosf"])
def test_host_entry_is_this_libm_f32(name):
    """a strided sample of the GPU test's own input set (tanf, sinf, cosf on [-8, 8], acosf on [-1.5, 1.5], as tools/check_libm_f32.cc)"""
    x = P.f32_inputs(name).view(np.float32)
    lim = {"tanf": 8.0, "sinf": 8.0, "cosf": 8.0, "acosf": 1.5}.get(name)
    if lim is not None:
        x = x[np.abs(x) <= lim]
    x = np.ascontiguousarray(x[:: max(1, len(x) // 30000)])
    got = P.host(name, x)[:, 0]
    want = _libm_f32(name, x)
    bad = ~P.same_bits(got, want)
    assert not bad.any(), (name, x[bad][:5], got[bad][:5], want[bad][:5])


def test_host_entry_is_this_libm_atan2f():
    yx = P.atan2f_inputs()
    yx = np.ascontiguousarray(np.concatenate([yx[:20000], yx[-4096:]]))
    got = P.host("atan2f", yx)[:, 0]
    f = yx.view(np.float32)
    want = _libm_f32("atan2f", f[:, 0], f[:, 1])
    bad = ~P.same_bits(got, want)
    assert not bad.any(), (f[bad][:5], got[bad][:5], want[bad][:5])


def test_host_entry_is_this_libm_f64():
    x = P.f64_sincos_inputs()
    x = np.ascontiguousarray(x[:: len(x) // 40000])
    assert P.same_bits(P.host("sin64", x)[:, 0], np.array([math.sin(v) for v in x])).all()
    assert P.same_bits(P.host("cos64", x)[:, 0], np.array([math.cos(v) for v in x])).all()
    sc = _libm.sincos
    sc.restype, sc.argtypes = None, [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    s, c = ctypes.c_double(), ctypes.c_double()
    want = []
    for v in x:
        sc(float(v), ctypes.byref(s), ctypes.byref(c))
        want.append((s.value, c.value))
    assert P.same_bits(P.host("sincos64", x), np.array(want)).all()
    e = P.f64_exp_inputs()
    e = np.ascontiguousarray(e[:: len(e) // 40000])
    assert P.same_bits(P.host("exp64", e)[:, 0], np.array([math.exp(v) for v in e])).all()


def test_libm_literals_are_listed():
    """every 32-bit literal libm_f32.h compares a word of its argument against is in F32_LITERALS under its function, on the line named"""
    import os
    import re
    lines = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "morb_slam_amd", "csrc", "libm_f32.h")).read().split("\n")
    start = {name: next(i for i, l in enumerate(lines) if fn in l)
             for name, fn in (("atanf", "float atanf_glibc(float"), ("acosf", "float acosf_glibc(float"), ("atan2f", "float atan2f_glibc(float"),
                              ("tanf", "float kernel_tanf_glibc(float"), ("sinf", "struct SinCosTab"))}
    masks = {0x7fffffff, 0x80000000, 0xfffff000, 0x7fc00000}
    found = 0
    for name, stop in (("atanf", "acosf"), ("acosf", "atan2f"), ("tanf", "sinf")):
        listed = {bits: where for bits, where in P.F32_LITERALS[name]}
        for i in range(start[name], start[stop]):
            if not re.search(r"\b(ix|hx)\b", lines[i]):
                continue
            for lit in re.findall(r"0x[0-9a-fA-F]{8}\b", lines[i].split("//")[0]):
                v = int(lit, 16)
                if v in masks:
                    continue
                assert v in listed, (name, i + 1, lit)
                assert str(i + 1) in re.split(r"[:, ]+", listed[v].split(":")[0] + ","), (name, i + 1, lit, listed[v])
                found += 1
    assert found >= 14, found


def test_scan_model_matches_lane_simulation():
    rng = np.random.default_rng(5)
    for trial in range(64):
        v = P.spread_doubles(rng) if trial % 2 else rng.integers(-1000, 1000, 64).astype(np.float64)
        if trial == 3:
            v = np.full(64, -0.0)
        brute = P.dpp_bruteforce([float(x) for x in v], lambda a, b: a + b, 0.0)
        model = P.sum_f64_model(v)
        assert np.float64(brute).view(np.uint64) == np.float64(model).view(np.uint64), trial
        rows = P.row_sum_f64_model(v)
        for r in range(4):
            w = [float(x) for x in v[16 * r: 16 * r + 16]]
            for sh in (1, 2, 4, 8):
                w = [w[i] + (w[i - sh] if i >= sh else 0.0) for i in range(16)]
            assert all(np.float64(rows[16 * r + i]).view(np.uint64) == np.float64(w[15]).view(np.uint64) for i in range(16))
        iv = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
        assert P.dpp_bruteforce([int(x) for x in iv], min, 0xFFFFFFFF) == int(iv.min())
        assert P.dpp_bruteforce([int(x) for x in iv], lambda a, b: a + b, 0) == int(iv.sum())


def test_spread_set_discriminates_the_order():
    """on the 2^0 .. 2^-60 sets a plain left-to-right sum differs from the scan's order; on integer-valued sets no order differs"""
    rng = np.random.default_rng(0x5CA)          # (the seed of the GPU test)
    differ = 0
    for _ in range(16):
        v = P.spread_doubles(rng)
        left = 0.0
        for x in v:
            left += float(x)
        differ += left != P.sum_f64_model(v)
    assert differ >= 12, differ
    iv = rng.integers(-2 ** 40, 2 ** 40, 64).astype(np.float64)
    assert float(sum(int(x) for x in iv)) == P.sum_f64_model(iv)


def test_branch_counts():
    """every branch named in the issue is entered by at least 100 inputs of the sets the GPU tests launch"""
    counts = {}
    for name, nbranch in (("R_to_q", 4), ("se3_exp", 2), ("exp_so3", 2), ("right_jacobian_so3", 2), ("inv_right_jacobian_so3", 2),
                          ("log_so3", 3), ("sim3_exp", 4)):
        br = P.lie_case(name)[4]
        counts[name] = np.bincount(br, minlength=nbranch).tolist()
        assert len(counts[name]) == nbranch and min(counts[name]) >= 100, (name, counts[name])
    print(counts)
    assert counts["R_to_q"] == [600, 156, 171, 123]            # trace > 0, then the largest diagonal x, y, z


@pytest.mark.parametrize("name", sorted(P.BOUNDS))
def test_lie_bounds_are_the_measured_ones(name):
    """BOUNDS[name][class] is the FP64 transcription's largest error against mpmath, rounded up: measured again, it lies in [value / 2, value]"""
    tr = P.lie_case(name)[3]
    got = P.class_errors(name, tr)
    assert set(got) == set(P.BOUNDS[name])
    for label, v in got.items():
        pin = P.BOUNDS[name][label]
        print(f"{name} {label}: measured {v:.3g} pinned {pin:.3g}")
        assert v <= pin and (v >= pin / 2 if pin > 0 else v == 0), (name, label, v, pin)


def test_dense_constants_are_the_measured_ones():
    """C_JACOBI, C_CLAMP, C_INVERT: 8 x the largest figure of the numpy transcriptions, rounded up"""
    worst = 0.0
    for m in P.JACOBI_SIZES:
        for kind in P.JACOBI_KINDS:
            for k in range(4):
                A = P.jacobi_case(m, kind, k)
                w, V = P.jacobi_numpy(A)
                worst = max([worst] + list(P.jacobi_check(A, w, V).values()))
    print("jacobi", worst)
    assert P.C_JACOBI / 2 <= 8 * worst <= P.C_JACOBI
    worst = 0.0
    for n in P.CLAMP_SIZES:
        for kind, S, e in P.clamp_cases(n):
            out = P.clamp_transcription(S, P.CLAMP_THR)
            assert (out.tobytes() == S.tobytes()) == (kind.split(",")[0] in ("above", "just above")), kind
            worst = max(worst, P.clamp_figure(S, out, P.CLAMP_THR))
    print("clamp", worst)
    assert P.C_CLAMP / 2 <= 8 * worst <= P.C_CLAMP
    worst = 0.0
    for n in P.INVERT_SIZES:
        for kind, A in P.invert_cases(n):
            ok, X = P.invert_numpy(A)
            assert ok == (kind != "singular"), (n, kind)
            if ok:
                worst = max(worst, P.inverse_figure(A, X))
    print("invert", worst)
    assert P.C_INVERT / 2 <= 8 * worst <= P.C_INVERT


def test_a_skipped_pair_is_out_of_bound():
    """what the row-Jacobi bound can see: one pair never rotated leaves figures far beyond C_JACOBI"""
    A = P.jacobi_case(9, "spd", 0)
    w, V = P.jacobi_numpy(A, skip_pair=(2, 5))
    assert max(P.jacobi_check(A, w, V).values()) > 1e6 * P.C_JACOBI
