"""The tier rule of projection.hip's window searches (morb_slam_amd/csrc/search_tier.h, compiled for the host) against its Python mirror
tests/search_tiers.py, which tests/test_search_tiers_gpu.py uses to say which tier each of its cases runs.  The grid holds every boundary
+-1: cap = qCap at the tier 1 / 2 and tier 2 / 3 limits, the 1200-feature frame (cap 1232) with the map-point counts at those limits, and
the 16-bit limit on both sizes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import search_tiers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("st") / "libst.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", out, os.path.join(NATIVE, "search_tier_check.cc")])
    L = C.CDLL(out)
    L.st_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.st_lds_bytes.restype = C.c_longlong
    L.st_tier.argtypes = [C.c_int, C.c_int, C.c_int]
    L.st_tiers.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return L


def _last_with(tier_of, lo, hi, want):
    """The largest x in [lo, hi] with tier_of(x) <= want (tier_of is monotone in x)."""
    assert tier_of(lo) <= want
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tier_of(mid) <= want: lo = mid
        else: hi = mid
    return lo


def test_boundaries_are_where_the_issue_table_puts_them():
    diag = lambda c: T.search_tier(c, c)
    assert _last_with(diag, 1, 4000, 1) == 1632 and _last_with(diag, 1, 4000, 2) == 2744
    at1232 = lambda q: T.search_tier(1232, q)
    assert _last_with(at1232, 1, 20000, 1) == 3208 and _last_with(at1232, 1, 20000, 2) == 5672
    # the frame capacities of the configurations the tests run: EuRoC stereo, KITTI stereo, 1080p, EuRoC mono initialisation
    assert [T.frame_cap(n) for n in (1200, 2000, 4000, 5000)] == [1232, 2032, 4032, 5032]
    assert [T.search_tier(c, c) for c in (1232, 2032, 4032, 5032)] == [1, 2, 3, 3]
    assert T.search_tier(1232, 4000) == 2 and T.search_tier(1232, 6000) == 3
    assert T.entry_tier("sim3", 1232, 100) == 3 and T.entry_tier("init", 1232) == 3 and T.entry_tier("last", 1232, serial=True) == 3


def _grid():
    pts = {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 1232, 2032, 4032, 5032, 8192, 20000, 65534, 65535, 65536, 70000}
    for b in (1632, 1633, 2744, 2745, 3208, 3209, 5672, 5673, 65535, 65536):
        pts.update(range(b - 5, b + 6))
    vals = sorted(p for p in pts if p > 0)
    caps, qs = np.meshgrid(np.array(vals, np.int32), np.array(vals, np.int32), indexing="ij")
    caps, qs = caps.ravel().copy(), qs.ravel().copy()
    rng = np.random.default_rng(17)                       # and a random cloud between the boundaries
    caps = np.concatenate([caps, rng.integers(1, 70000, 4000).astype(np.int32), rng.integers(1500, 3000, 4000).astype(np.int32)])
    qs = np.concatenate([qs, rng.integers(1, 70000, 4000).astype(np.int32), rng.integers(1, 7000, 4000).astype(np.int32)])
    return caps, qs


@pytest.mark.parametrize("serial", [0, 1])
def test_header_equals_mirror(st, serial):
    caps, qs = _grid()
    got = np.zeros(len(caps), np.int32)
    st.st_tiers(len(caps), caps.ctypes.data, qs.ctypes.data, serial, got.ctypes.data)
    exp = np.array([T.search_tier(int(c), int(q), bool(serial)) for c, q in zip(caps, qs)], np.int32)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(caps[i]), int(qs[i]), int(got[i]), int(exp[i])) for i in bad[:10]]
    if not serial:
        assert set(np.unique(got)) == {1, 2, 3}
    else:
        assert (got == 3).all()


def test_lds_bytes_and_named_boundaries(st):
    for cap, q in [(1, 1), (1232, 1232), (1632, 1632), (1633, 1633), (2744, 2744), (2745, 2745), (1232, 3208), (1232, 3209), (1232, 5672),
                   (1232, 5673), (65535, 1), (4032, 4032)]:
        for wd in (0, 1):
            assert st.st_lds_bytes(cap, q, wd) == T.search_lds_bytes(cap, q, bool(wd)), (cap, q, wd)
    named = {(1632, 1632): 1, (1633, 1633): 2, (2744, 2744): 2, (2745, 2745): 3, (1232, 3208): 1, (1232, 3209): 2, (1232, 5672): 2,
             (1232, 5673): 3, (1232, 65535): 3, (1232, 65536): 3, (65535, 1): 3, (65536, 1): 3, (100, 65535): 3, (100, 65536): 3}
    for (cap, q), t in named.items():
        assert st.st_tier(cap, q, 0) == t == T.search_tier(cap, q), (cap, q)
