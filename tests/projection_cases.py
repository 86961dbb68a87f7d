"""Constructed frames that put the projection searches and the frustum test of csrc/projection.hip ON their decision thresholds.

Every other projection test takes its keypoints from the extractor and its map points from back-projection, where a feature exactly r from the
window centre, a projection exactly on maxX, a Hamming distance of exactly 100 or a histogram bin of exactly a tenth of the largest never
occur.  Here the keypoint records are written directly (KP_DTYPE, no image) on a camera chosen so that float32 arithmetic is exact:
  image 512 x 384 (gridInvW = gridInvH = 0.125), fx = fy = 256, cx = 256, cy = 192, mbf = 32; poses are the identity; points sit at depth
  1, 2 or 4; pyramids (1.2, 8 levels), (1.5, 4), (2.0, 3) through make_frame_params.
Each builder recomputes the quantity it aims at in np.float32, operation by operation as the kernel writes it, and asserts that the threshold
is hit exactly or that its two inputs are adjacent floats (np.nextafter) on either side of it: a case that misses its threshold fails when it is
built.  Descriptors get exact Hamming distances by flipping a chosen number of bits of a base descriptor.  SearchByProjection(F, MapPoints)
is fed its tracking tables (projX, projY, projXR, level, viewCos, depth, inView) directly, so the search cases do not depend on the frustum.

A problem is a dict of host arrays: the inputs of ONE oracle call, `expect` = the outcome written by hand from the reference lines cited next
to each sub-case (never computed by the oracle), `differ` = pairs of output rows on the two sides of a threshold (their outcomes must differ, so
no case is vacuous) and `classes` = sub-cases per case class.  Sub-cases of one problem sit at their own anchors of a 56 x 48 px lattice, far
outside each other's windows.  test_projection_cases_cpu.py checks oracle == expect; test_projection_cases_gpu.py runs the same problems,
batched with an empty and a one-feature frame, on every implementation tier of the kernels against the oracle.

Unreachable, and what stands in its place:
  * one ulp below minX = 0 (and minY = 0): the neighbour of 0 is a denormal, and u = fx * x / z + cx is a sum with 256, so the closest value
    below 0 that any input reaches is -2^-15 (one ulp of the addend).  That value is used.
  * Pc.z = -0.0 in SearchByProjection(Cur, Last) and the keyframe projections: Eigen's quaternion rotation adds +0 terms to v.z, and
    -0 + +0 = +0, so with an identity quaternion no input gives x3Dc.z = -0.0 (found by trying every sign of the zero operands,
    _last_minus_zero_reachable()).  The frustum's matrix form does reach it (X0, X1 < 0, t.z = -0.0) and is tested there.
  * exact equality in the epipolar-line test and in Fuse's chi-square gate: 3.84 * sigma2, 5.99 and 7.8 are doubles that are not float32
    values, so `dsqr == bound` has no float32 solution; the two float32 values adjacent to the bound (chi-square) and the two nearest values
    that adjacent keypoint coordinates reach (epipolar line) are used.
  * float products, worked out: 0.8f * 50 is 40.0000006 exactly and 40.0f in float32; 0.9f * 50 is 44.9999988 exactly and 45.0f in float32.  The
    reference multiplies in float (ORBmatcher.cc:121, :487, :653), so in SearchByProjection(F, MapPoints) 45 against 50 at ratio 0.9 is ACCEPTED
    (`45 > 45.0f` is false; a double product would reject it) and 46 is its rejected side; 40 against 50 at 0.8 is accepted either way and 41 is
    rejected.  SearchByProjection(KF, Scw) with ratioHamming 0.9 accepts up to 45, not 44, for the same reason.  SearchForInitialization's strict
    `40 < 50 * 0.8f` is false in float32 and true in exact arithmetic.  (The issue behind these cases states the 0.9 outcomes for exact arithmetic;
    the oracle, the kernels and the reference's own expressions agree on the float32 ones, which are asserted here.)
  * ComputeThreeMaxima exists three times in projection.hip, not four: k_resolve, k_search and k_rot_filter12 (SearchForTriangulation's
    k_triangulation writes the bins and k_rot_filter12 filters them).  The histogram problems run through all three.
  * the rotation histogram has 30 bins but factor = 1 / HISTO_LENGTH maps rot in [0, 360) to bins 0 .. 12 only (the reference's own
    arithmetic, ORBmatcher.cc:1625-1632): the problems use bins 0 .. 12.
"""
import itertools

import numpy as np

import oracle_lib as O
from oracle_lib import KP_DTYPE

F32 = np.float32
W, H, FX, FY, CX, CY, MBF, MB = 512, 384, 256.0, 256.0, 256.0, 192.0, 32.0, 0.125
PYRAMIDS = {"p12": (1.2, 8), "p15": (1.5, 4), "p20": (2.0, 3)}
CACHE_PYRAMIDS = {"p13": (1.3, 6), "p11": (1.1, 8), "p17": (1.7, 5)}     # with PYRAMIDS: six, more than the 4-way constant cache holds
TH_HIGH, TH_LOW = 100, 50
IDENTITY7 = np.array([0, 0, 0, 1, 0, 0, 0], F32)


def up(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(np.inf))
    return x


def dn(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(-np.inf))
    return x


def scale_factors(pyr):
    """mvScaleFactor as ORBextractor builds it (ORBextractor.cc:412-418): a running float product."""
    s, n = {**PYRAMIDS, **CACHE_PYRAMIDS}[pyr]
    sf = [F32(1.0)]
    for _ in range(n - 1):
        sf.append(F32(sf[-1] * F32(s)))
    return np.array(sf, F32)


_PARAMS = {}


def params(pyr):
    from morb_slam_amd.capi import make_frame_params
    if pyr not in _PARAMS:
        sf = scale_factors(pyr)
        P = make_frame_params(W, H, FX, FY, CX, CY, MBF, MB, [float(v) for v in sf], [float(F32(v * v)) for v in sf],
                              scale_factor={**PYRAMIDS, **CACHE_PYRAMIDS}[pyr][0])
        assert P.gridInvW == 0.125 and P.gridInvH == 0.125 and (P.minX, P.minY, P.maxX, P.maxY) == (0.0, 0.0, 512.0, 384.0)
        _PARAMS[pyr] = P
    return _PARAMS[pyr]


def sigma2(pyr):
    sf = scale_factors(pyr)
    return (sf * sf).astype(F32)


# ---- descriptors with exact distances --------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(20261021)


def base_desc():
    return _rng.integers(0, 256, 32, dtype=np.uint8)


def flip(d, n, start=0):
    """d with bits [start, start + n) flipped: Hamming distance n from d."""
    out = d.copy()
    for b in range(start, start + n):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def cell(x):
    """PosInGrid's std::round((x - 0) * 0.125f): half away from zero, in float32."""
    v = F32(F32(x) * F32(0.125))
    return int(np.sign(v) * np.floor(np.abs(v) + F32(0.5)))


def rot_bin(rot):
    """(int)round(rot * (1.0f / 30)) with the 360 added below zero and bin 30 folded to 0 (ORBmatcher.cc:1625-1632)."""
    rot = F32(rot)
    if rot < 0:
        rot = F32(rot + F32(360.0))
    v = F32(rot * F32(F32(1.0) / F32(30)))
    b = int(np.floor(v + F32(0.5))) if v >= 0 else -int(np.floor(-v + F32(0.5)))
    return 0 if b == 30 else b


class Frame:
    """The searched frame: keypoint records, descriptors, uRight, a per-feature flag (blocked / has a map point) and the in/out table on entry."""

    def __init__(self):
        self.rows = []
        self._anchor = 0
        self.expect = {}       # output row -> value written by hand
        self.differ = []       # (row a, row b): the two sides of a threshold
        self.classes = {}

    def anchor(self):
        i = self._anchor
        self._anchor += 1
        assert i < 56, "a frame holds 56 anchors"
        return F32(42 + 56 * (i % 8)), F32(42 + 48 * (i // 8))

    def feat(self, x, y, octave=0, desc=None, ur=-1.0, flag=0, init=-1, angle=0.0):
        self.rows.append((F32(x), F32(y), int(octave), F32(angle), base_desc() if desc is None else desc, F32(ur), int(flag), int(init)))
        assert len(self.rows) <= 128
        return len(self.rows) - 1

    def count(self, cls, n=1):
        self.classes[cls] = self.classes.get(cls, 0) + n

    def frame_arrays(self):
        n = len(self.rows)
        k = np.zeros(n, KP_DTYPE)
        k["x"] = [r[0] for r in self.rows]; k["y"] = [r[1] for r in self.rows]; k["octave"] = [r[2] for r in self.rows]
        k["angle"] = [r[3] for r in self.rows]; k["size"] = 31.0; k["response"] = 1.0; k["class_id"] = -1
        d = np.stack([r[4] for r in self.rows]) if n else np.zeros((0, 32), np.uint8)
        return dict(k=k, d=d.astype(np.uint8), ur=np.array([r[5] for r in self.rows], F32), flag=np.array([r[6] for r in self.rows], np.uint8),
                    init=np.array([r[7] for r in self.rows], np.int32))

    def expected_table(self, init):
        e = init.copy()
        for f, q in self.expect.items():
            e[f] = q
        return e


def keypoints(rows):
    """KP_DTYPE records from (x, y, octave, angle) rows."""
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, o, a) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"] = x, y, o, a
    k["size"] = 31.0; k["response"] = 1.0; k["class_id"] = -1
    return k


def backproject(u, v, z):
    """The camera point at depth z that the pinhole formula fx * X / Z + cx sends to (u, v) EXACTLY (asserted)."""
    z = F32(z)
    X = np.array([F32(F32(F32(u) - F32(CX)) * z) / F32(FX), F32(F32(F32(v) - F32(CY)) * z) / F32(FY), z], F32)
    uu = F32(F32(F32(FX) * X[0]) / X[2]) + F32(CX); vv = F32(F32(F32(FY) * X[1]) / X[2]) + F32(CY)
    assert uu == F32(u) and vv == F32(v), ("no exact back-projection", u, v, z, uu, vv)
    return X


def solve(fn, target, start, steps=64):
    """The float32 x near `start` with fn(x) == target: walks nextafter both ways; a threshold that no input reaches fails here."""
    lo = hi = F32(start)
    for _ in range(steps):
        if fn(lo) == target:
            return lo
        if fn(hi) == target:
            return hi
        lo, hi = dn(lo), up(hi)
    raise AssertionError(("threshold not reachable", target, start))


# =========================================================================================================================================
# Frame::isInFrustum (Frame.cc:611-678) + MapPoint::PredictScale (MapPoint.cc:552-566)
# =========================================================================================================================================
class FrustumScene:
    def __init__(self, name, pyr="p12", t=(0, 0, 0), Ow=(0, 0, 0), cosLimit=0.5):
        self.name, self.pyr, self.cosLimit = name, pyr, cosLimit
        self.R = np.eye(3, dtype=F32).reshape(9); self.t = np.array(t, F32); self.Ow = np.array(Ow, F32)
        self.rows, self.expect, self.differ, self.classes, self.level, self.proj, self.nan_rows = [], {}, [], {}, {}, {}, []

    def point(self, P, normal=None, maxD=4.0, minD=0.0, inView=None, level=None, proj=None):
        P = np.array(P, F32)
        PO = P - self.Ow
        if normal is None:       # along the viewing ray, unit length where that is exact: viewCos = 1 for axis points
            normal = PO
        self.rows.append((P, np.array(normal, F32), F32(maxD), F32(minD)))
        i = len(self.rows) - 1
        if inView is not None:
            self.expect[i] = int(inView)
        if level is not None:
            self.level[i] = level
        if proj is not None:
            self.proj[i] = (F32(proj[0]), F32(proj[1]))
        return i

    def Pc(self, P):
        """(R0 X0 + R1 X1) + R2 X2 + t, row by row, as k_frustum and the oracle write it."""
        R, P = self.R, np.array(P, F32)
        return np.array([F32(F32(F32(F32(R[3 * r] * P[0]) + F32(R[3 * r + 1] * P[1])) + F32(R[3 * r + 2] * P[2])) + self.t[r]) for r in range(3)], F32)

    def uv(self, P):
        with np.errstate(all="ignore"):
            c = self.Pc(P)
            return F32(F32(F32(FX) * c[0]) / c[2]) + F32(CX), F32(F32(F32(FY) * c[1]) / c[2]) + F32(CY)

    def dist(self, P):
        PO = np.array(P, F32) - self.Ow
        return np.sqrt(F32(F32(F32(PO[0] * PO[0]) + F32(PO[1] * PO[1])) + F32(PO[2] * PO[2])))

    def count(self, cls, n=1):
        self.classes[cls] = self.classes.get(cls, 0) + n

    def problem(self):
        a = [np.stack([r[j] for r in self.rows]) for j in range(4)]
        n = len(self.rows)
        return dict(entry="frustum", name=self.name, pyr=self.pyr, R=self.R, t=self.t, Ow=self.Ow, Pw=a[0], normal=a[1], maxD=a[2], minD=a[3],
                    cosLimit=self.cosLimit, expect=np.array([self.expect[i] for i in range(n)], np.uint8), level=dict(self.level),
                    proj=dict(self.proj), differ=list(self.differ), classes=dict(self.classes), nan_rows=list(self.nan_rows))


def frustum_main():
    S = FrustumScene("frustum_main", "p12")
    # -- image bounds, closed interval (Frame.cc:629-632: `u < mnMinX || u > mnMaxX` returns false)
    ulp0 = F32(-2.0 ** -15)
    for axis, lo, hi, c in ((0, 0.0, 512.0, CX), (1, 0.0, 384.0, CY)):
        other = (CY, CX)[axis]
        def P_of(a, axis=axis):
            return (a, 0.0, 1.0) if axis == 0 else (0.0, a, 1.0)
        def u_of(a, axis=axis):
            return S.uv(P_of(a))[axis]
        a_hi = solve(u_of, F32(hi), (hi - c) / 256.0); a_hi_out = solve(u_of, up(hi), (hi - c) / 256.0)
        a_lo = solve(u_of, F32(lo), (lo - c) / 256.0); a_lo_out = solve(u_of, ulp0, (lo - c) / 256.0)
        assert u_of(a_hi) == F32(hi) and u_of(a_hi_out) == up(hi) and u_of(a_lo) == F32(lo) and u_of(a_lo_out) < 0
        pr = lambda val, axis=axis, other=other: (val, other) if axis == 0 else (other, val)
        i0 = S.point(P_of(a_hi), inView=1, proj=pr(hi)); i1 = S.point(P_of(a_hi_out), inView=0)
        i2 = S.point(P_of(a_lo), inView=1, proj=pr(lo)); i3 = S.point(P_of(a_lo_out), inView=0)
        S.differ += [(i0, i1), (i2, i3)]
        S.count("frustum.bounds", 4)
    # -- distance (Frame.cc:640-645): dist < 0.8f * minDist or dist > 1.2f * maxDist returns false
    P2 = (0.0, 0.0, 2.0)
    assert S.dist(P2) == F32(2.0)
    mn = lambda m: F32(F32(0.8) * F32(m)); mx = lambda m: F32(F32(1.2) * F32(m))
    m_eq, m_up, m_dn = solve(mn, F32(2.0), 2.5), solve(mn, up(2.0), 2.5), solve(mn, dn(2.0), 2.5)
    a = S.point(P2, maxD=4.0, minD=m_eq, inView=1); b = S.point(P2, maxD=4.0, minD=m_up, inView=0); c_ = S.point(P2, maxD=4.0, minD=m_dn, inView=1)
    S.differ.append((a, b)); S.differ.append((c_, b))
    M_eq, M_up, M_dn = solve(mx, F32(2.0), 2.0 / 1.2), solve(mx, up(2.0), 2.0 / 1.2), solve(mx, dn(2.0), 2.0 / 1.2)
    a = S.point(P2, maxD=M_eq, inView=1); b = S.point(P2, maxD=M_dn, inView=0); c_ = S.point(P2, maxD=M_up, inView=1)
    S.differ.append((a, b)); S.differ.append((c_, b))
    S.count("frustum.distance", 6)
    # -- viewing angle (Frame.cc:648-653): viewCos = PO . Pn / dist < viewingCosLimit returns false
    n_eq = (0.0, 0.0, 0.5); n_lo = (0.0, 0.0, dn(0.5))
    assert F32(F32(F32(2.0) * F32(0.5)) / F32(2.0)) == F32(0.5) and F32(F32(F32(2.0) * dn(0.5)) / F32(2.0)) == dn(0.5)
    a = S.point(P2, normal=n_eq, inView=1); b = S.point(P2, normal=n_lo, inView=0)
    S.differ.append((a, b))
    S.count("frustum.viewcos", 2)
    return S.problem()


def frustum_depth():
    """Pc.z at +0.0, -0.0, the smallest negative and the smallest positive normal (Frame.cc:621-623: `PcZ < 0.0f` returns false, so both zeros
    go on and divide).  Ow = (0, 0, -1) keeps dist = 1 whatever Pc.z is; tcw.z = -0.0 lets Pc.z = -0.0 survive the sum."""
    tiny = np.finfo(F32).tiny
    S = FrustumScene("frustum_depth", "p12", t=(0.0, 0.0, -0.0), Ow=(0.0, 0.0, -1.0))
    with np.errstate(all="ignore"):
        # +0.0 and -0.0 off the axis: u = fx * x / (+-0) is infinite, out of bounds either way
        pz = S.Pc((-1.0, -1.0, 0.0))[2]; nz = S.Pc((-1.0, -1.0, -0.0))[2]
        assert pz == 0 and not np.signbit(pz), "Pc.z = +0.0 not reached"
        assert nz == 0 and np.signbit(nz), "Pc.z = -0.0 not reached"
        S.point((-1.0, -1.0, 0.0), normal=(0, 0, 1), inView=0)
        S.point((-1.0, -1.0, -0.0), normal=(0, 0, 1), inView=0)
        # on the axis 0 / 0 = NaN passes both bounds tests (every comparison with NaN is false) and the point is IN VIEW with NaN projections
        for z in (0.0, -0.0):
            assert np.isnan(S.uv((0.0, 0.0, z))[0])
        # (X0 = X1 = -0.0 keeps the sum at -0.0: 0 * -0 = -0)
        assert np.signbit(S.Pc((-0.0, -0.0, -0.0))[2]) and np.isnan(S.uv((-0.0, -0.0, -0.0))[0])
        i = S.point((0.0, 0.0, 0.0), normal=(0, 0, 1), inView=1); j = S.point((-0.0, -0.0, -0.0), normal=(0, 0, 1), inView=1)
        S.nan_rows += [i, j]
    a = S.point((0.0, 0.0, -tiny), normal=(0, 0, 1), inView=0)
    b = S.point((0.0, 0.0, tiny), normal=(0, 0, 1), inView=1, proj=(CX, CY))
    S.differ.append((a, b))
    S.count("frustum.depth_sign", 6)
    return S.problem()


def predict_level(pyr, ratio):
    """The oracle's PredictScale for dist = 1, maxDist = ratio (one point through orc_is_in_frustum)."""
    P = params(pyr)
    F = O.make_frame(P, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), None)
    o = O.is_in_frustum(F, np.eye(3, dtype=F32), np.zeros(3, F32), np.zeros(3, F32), np.array([[0, 0, 1]], F32), np.array([[0, 0, 1]], F32),
                        np.array([ratio], F32), np.zeros(1, F32), 0.5)
    assert o["inView"][0] == 1
    return int(o["level"][0])


def level_boundary(pyr, n):
    """The largest float32 ratio whose predicted level is <= n, by bisection on the oracle's level over the float32 bit patterns."""
    lo, hi = F32(1.0), F32(64.0)
    assert predict_level(pyr, lo) <= n < predict_level(pyr, hi)
    a, b = int(lo.view(np.int32)), int(hi.view(np.int32))
    while b - a > 1:
        m = (a + b) // 2
        if predict_level(pyr, np.int32(m).view(F32)) <= n:
            a = m
        else:
            b = m
    return np.int32(a).view(F32)


def frustum_predict_scale(pyr):
    """dist = 1 exactly (P = (0, 0, 1), Ow = 0), so ratio = maxDist / dist = maxDist: per level n the largest maxDist predicted n and the next
    float up (predicted n + 1), a ratio below 1 (level 0) and one far above the top (clamped)."""
    s, nl = {**PYRAMIDS, **CACHE_PYRAMIDS}[pyr]
    S = FrustumScene("predict_scale_" + pyr, pyr)
    P1 = (0.0, 0.0, 1.0)
    assert S.dist(P1) == F32(1.0)
    bounds = []
    for n in range(nl - 1):
        b = level_boundary(pyr, n)
        # MapPoint.cc:552-566: level = ceil(log(ratio) / logScaleFactor), so the boundary is s^n up to the rounding of logf and of the quotient:
        # a relative error of 2 * 2^-23 in the logarithm moves the ratio by 2^-22 * n * ln(s) <= 3.1e-7 (n ln s <= ln 1.2^7); 1e-6 bounds it
        assert abs(float(b) / float(F32(s)) ** n - 1.0) < 1e-6, (pyr, n, b)
        i = S.point(P1, normal=(0, 0, 1), maxD=b, inView=1, level=n, proj=(CX, CY)); j = S.point(P1, normal=(0, 0, 1), maxD=up(b), inView=1, level=n + 1)
        S.differ.append((i, j))
        bounds.append(b)
    S.point(P1, normal=(0, 0, 1), maxD=0.9, inView=1, level=0)            # ratio < 1: nScale < 0 -> 0 (1.2f * 0.9 >= dist keeps it in range)
    S.point(P1, normal=(0, 0, 1), maxD=1000.0, inView=1, level=nl - 1)     # far above the top: clamped to nlevels - 1
    if s == 2.0:
        S.point(P1, normal=(0, 0, 1), maxD=4.0, inView=1)                  # logf(4) / logf(2) need not be 2: whatever the oracle says, bit for bit
    S.count("frustum.predict_scale", 2 * (nl - 1) + 2)
    p = S.problem()
    p["bounds"] = bounds
    return p


# =========================================================================================================================================
# ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints)  (ORBmatcher.cc:42-209)
# =========================================================================================================================================
class MpsScene(Frame):
    def __init__(self, name, pyr="p12", th=1.0, nnratio=0.8, bFar=False, thFar=0.0):
        super().__init__()
        self.name, self.pyr, self.th, self.nnratio, self.bFar, self.thFar = name, pyr, th, nnratio, bFar, thFar
        self.sf = scale_factors(pyr)
        self.q, self.ghost = [], []

    def r(self, lv, viewCos=0.5):
        """RadiusByViewingCos (:211-216, the comparison is in double), `if (bFactor) r *= th`, then r * mvScaleFactors[level] (:96-104)."""
        r = F32(2.5) if float(F32(viewCos)) > 0.998 else F32(4.0)
        if float(F32(self.th)) != 1.0:
            r = F32(r * F32(self.th))
        return F32(r * self.sf[lv])

    def query(self, x, y, lv, desc, viewCos=0.5, xr=-1.0, depth=1.0, inView=1, isBad=0, hasObs=1, ghost=False):
        row = (F32(x), F32(y), int(lv), desc, F32(viewCos), F32(xr), F32(depth), int(inView), int(isBad), int(hasObs))
        (self.ghost if ghost else self.q).append(row)
        assert len(self.q) + len(self.ghost) <= 128
        return -1 if ghost else len(self.q) - 1

    def _tables(self, rows):
        n = len(rows)
        g = lambda j, dt: np.array([r[j] for r in rows], dt)
        return dict(projX=g(0, F32), projY=g(1, F32), level=g(2, np.int32), mpDesc=(np.stack([r[3] for r in rows]) if n else np.zeros((0, 32), np.uint8)),
                    viewCos=g(4, F32), projXR=g(5, F32), depth=g(6, F32), inView=g(7, np.uint8), isBad=g(8, np.uint8), hasObs=g(9, np.uint8))

    def problem(self):
        fa = self.frame_arrays()
        return dict(entry="mps", name=self.name, pyr=self.pyr, th=self.th, nnratio=self.nnratio, bFar=self.bFar, thFar=self.thFar, **fa,
                    q=self._tables(self.q), ghost=self._tables(self.ghost), expect=self.expected_table(fa["init"]), differ=list(self.differ),
                    classes=dict(self.classes))


def _mps_window(S, lv, exact=True):
    """GetFeaturesInArea's `fabs(distx) < factorX && fabs(disty) < factorY` (Frame.cc:795-799): a feature at exactly r is rejected although its
    descriptor is the query's; one ulp inside, the other feature is the only candidate and is matched."""
    r = S.r(lv)
    for axis, sign in itertools.product((0, 1), (1, -1)):
        x, y = S.anchor()
        B = base_desc()
        c = (x, y)[axis]
        out_, in_ = (up, dn) if sign > 0 else (dn, up)
        e = F32(c + sign * r)
        while abs(F32(e - c)) < r:
            e = out_(e)
        while abs(F32(in_(e) - c)) >= r:
            e = in_(e)
        i = in_(e)
        # exact wherever r is a float32 the sum c + r holds (every level of the 1.5 and 2.0 pyramids, level 0 of 1.2); else the adjacent pair around r
        assert abs(F32(i - c)) < r <= abs(F32(e - c)) and out_(i) == e and (not exact or abs(F32(e - c)) == r), "window edge not hit"
        q = S.query(x, y, lv, B)
        fe = S.feat(e, y, lv, B) if axis == 0 else S.feat(x, e, lv, B)
        fi = S.feat(i, y, lv, flip(B, 10)) if axis == 0 else S.feat(x, i, lv, flip(B, 10))
        S.expect[fi] = q
        S.differ.append((fe, fi))
        S.count("mps.window")


def _mps_viewcos(S):
    """`if (viewCos > 0.998) return 2.5; else return 4.0` (:211-216) with a float viewCos against the DOUBLE 0.998: float32(0.998) is above it."""
    hi = F32(0.998); lo = dn(hi)
    assert float(hi) > 0.998 and float(lo) <= 0.998 and not (hi > F32(0.998))
    r_small, r_big = S.r(0, hi), S.r(0, lo)
    dx = F32((r_small + r_big) / 2)
    assert r_small < dx < r_big
    out = []
    for vc in (hi, lo):
        x, y = S.anchor()
        B = base_desc()
        q = S.query(x, y, 0, B, viewCos=vc)
        f_between = S.feat(x + dx, y, 0, B)                 # between the two radii, the query's own descriptor
        f_near = S.feat(x + 1, y, 0, flip(B, 10))
        S.expect[f_near if vc == hi else f_between] = q     # radius 4: best 0, second 10 at the same level: 0 > 0.8 * 10 is false
        out.append(f_between)
    S.differ.append(tuple(out))
    S.count("mps.radius_by_viewcos", 2)


def _mps_far(S):
    """`if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;` (:67-68): equal is kept."""
    assert S.bFar
    out = []
    for depth in (F32(S.thFar), up(S.thFar)):
        x, y = S.anchor()
        B = base_desc()
        q = S.query(x, y, 0, B, depth=depth)
        f = S.feat(x + 1, y, 0, flip(B, 7))
        if depth == F32(S.thFar):
            S.expect[f] = q
        out.append(f)
    S.differ.append(tuple(out))
    S.count("mps.far_points", 2)


def _mps_dropped(S):
    """isBad (:70-71), mbTrackInView false (:64-65) and a row at or beyond nMP: none of them may match a feature that carries its descriptor."""
    x, y = S.anchor(); B = base_desc(); q = S.query(x, y, 0, B); f_ok = S.feat(x + 1, y, 0, B); S.expect[f_ok] = q
    for kw in (dict(isBad=1), dict(inView=0), dict(ghost=True)):
        x, y = S.anchor(); B = base_desc()
        S.query(x, y, 0, B, **kw)
        f = S.feat(x + 1, y, 0, B)
        S.differ.append((f_ok, f))
    S.count("mps.dropped_queries", 3)


def _mps_grid_rounding(S):
    """Frame::PosInGrid (Frame.cc:809-820) is round(), half AWAY from zero.  A feature with (x - minX) * gridInvW == 12.5 lies in column 13, so
    with equal distances the feature of column 12 is met first although its index is higher (the walk is column, row, index); round-half-even would
    put both in column 12 and hand the match to the lower index.  The same in y, and x = -4 (-0.5 -> -1: never in the grid; half-even: column 0)."""
    lv = 1
    r = S.r(lv)
    assert r > 4
    for axis, c in ((0, F32(100.0)), (1, F32(356.0))):
        assert F32(c * F32(0.125)) % 1 == 0.5 and int(F32(c * F32(0.125))) % 2 == 0 and cell(c) == int(c) // 8 + 1 and cell(c - 2) == int(c) // 8
        B = base_desc()
        if axis == 0:
            q = S.query(c - 1, 362.0, lv, B)
            fa = S.feat(c, 362.0, lv, flip(B, 10)); fb = S.feat(c - 2, 362.0, lv - 1, flip(B, 10, 10))
        else:
            q = S.query(300.0, c - 1, lv, B)
            fa = S.feat(300.0, c, lv, flip(B, 10)); fb = S.feat(300.0, c - 2, lv - 1, flip(B, 10, 10))
        S.expect[fb] = q          # different levels, so the ratio rule does not apply (:118-121)
        S.differ.append((fa, fb))
        S.count("mps.grid_rounding")
    assert F32(F32(-4.0) * F32(0.125)) == F32(-0.5) and cell(-4.0) == -1
    B = base_desc()
    q = S.query(0.0, 210.0, lv, B)
    f_out = S.feat(-4.0, 210.0, lv, B); f_in = S.feat(1.0, 210.0, lv, flip(B, 10))
    S.expect[f_in] = q
    S.differ.append((f_out, f_in))
    S.count("mps.grid_rounding")


def _mps_outside_grid(S):
    """posX == 64 (x >= 508) or posY == 48 (y >= 380) never enters mGrid (Frame.cc:816-817), so such a feature is never matched although it lies inside
    the window and inside the image bounds."""
    assert cell(508.0) == 64 and cell(dn(508.0)) == 63 and cell(512.0) == 64 and cell(380.0) == 48 and cell(dn(380.0)) == 47 and cell(384.0) == 48
    B = base_desc(); q = S.query(506.0, 114.0, 0, B)
    f0 = S.feat(508.0, 114.0, 0, B); f1 = S.feat(dn(508.0), 114.0, 0, flip(B, 10))
    S.expect[f1] = q; S.differ.append((f0, f1))
    B = base_desc(); S.query(510.0, 162.0, 0, B); S.feat(512.0, 162.0, 0, B)           # x == maxX: |dx| = 2 < r, never matched
    B = base_desc(); q = S.query(238.0, 378.0, 0, B)
    f0 = S.feat(238.0, 380.0, 0, B); f1 = S.feat(238.0, dn(380.0), 0, flip(B, 10))
    S.expect[f1] = q; S.differ.append((f0, f1))
    B = base_desc(); S.query(182.0, 382.0, 0, B); S.feat(182.0, 384.0, 0, B)
    S.count("mps.outside_grid", 4)


def _mps_cell_range(S):
    """GetFeaturesInArea's cell range (Frame.cc:752-775): floor / ceil ends that are exact integers, windows clipped at each border, and windows
    wholly outside (nMinCellX >= 64, nMaxCellX < 0, the same in y: return before any feature is looked at)."""
    r = S.r(0)
    assert r == 4
    B = base_desc(); q = S.query(164.0, 68.0, 0, B)
    for v in (F32(164 - 4), F32(164 + 4), F32(68 - 4), F32(68 + 4)):
        assert F32(v * F32(0.125)) % 1 == 0
    f_edge = S.feat(160.0, 68.0, 0, B); f_lo = S.feat(up(160.0), up(64.0), 0, flip(B, 10)); f_hi = S.feat(dn(168.0), dn(72.0), 0, flip(B, 5))
    assert (cell(up(160.0)), cell(up(64.0)), cell(dn(168.0)), cell(dn(72.0))) == (20, 8, 21, 9)
    S.expect[f_hi] = q            # 5 against 10 at one level: 5 > 0.8 * 10 is false
    S.differ.append((f_edge, f_hi))
    for qx, qy, fx_, fy_ in ((2.0, 258.0, 1.0, 258.0), (505.0, 258.0, 503.0, 258.0), (294.0, 2.0, 294.0, 1.0), (294.0, 377.0, 294.0, 375.0)):
        B = base_desc(); q = S.query(qx, qy, 0, B); f = S.feat(fx_, fy_, 0, flip(B, 10)); S.expect[f] = q
        assert 0 <= cell(fx_) < 64 and 0 <= cell(fy_) < 48
    for qx, qy, fx_, fy_ in ((520.0, 258.0, 518.0, 258.0), (-13.0, 306.0, -12.0, 306.0), (350.0, 400.0, 350.0, 399.0), (350.0, -13.0, 350.0, -12.0)):
        B = base_desc(); S.query(qx, qy, 0, B); S.feat(fx_, fy_, 0, B)
    assert int(np.floor(F32(F32(520.0 - 4) * F32(0.125)))) >= 64 and int(np.ceil(F32(F32(-13.0 + 4) * F32(0.125)))) < 0
    assert int(np.floor(F32(F32(400.0 - 4) * F32(0.125)))) >= 48
    S.count("mps.cell_range", 9)


def _mps_levels(S, lvs):
    """GetFeaturesInArea(.., nPredictedLevel - 1, nPredictedLevel) (:96-104): octaves lv - 1 and lv only.  lv == 0 gives minLevel -1, and the levels are
    still checked because maxLevel >= 0 (Frame.cc:777)."""
    nl = len(S.sf)
    for lv in lvs:
        ins, outs = [], []
        for fo in range(lv - 2, lv + 2):
            if not 0 <= fo < nl:
                continue
            x, y = S.anchor(); B = base_desc()
            q = S.query(x, y, lv, B)
            f = S.feat(x + 1, y, fo, flip(B, 10))
            if fo in (lv - 1, lv):
                S.expect[f] = q; ins.append(f)
            else:
                outs.append(f)
            S.count("mps.levels")
        S.differ += [(ins[0], o) for o in outs]


def _mps_stereo(S):
    """`if (F.mvuRight[idx] > 0) { er = fabs(mTrackProjXR - mvuRight[idx]); if (er > r * scaleFactor) continue; }` (:108-113): er == r is kept, uRight == 0
    and uRight < 0 are not gated at all."""
    r = S.r(0)
    xr = F32(100.0)
    kept = F32(xr + r); gone = up(kept)
    assert abs(F32(xr - kept)) == r and abs(F32(xr - gone)) > r
    fs = {}
    for name, ur in (("kept", kept), ("gone", gone), ("zero", F32(0.0)), ("neg", F32(-1.0)), ("tiny", F32(1e-30))):
        x, y = S.anchor(); B = base_desc()
        q = S.query(x, y, 0, B, xr=xr)
        fs[name] = S.feat(x + 1, y, 0, flip(B, 10), ur=ur)
        if name not in ("gone", "tiny"):
            S.expect[fs[name]] = q
    S.differ += [(fs["kept"], fs["gone"]), (fs["zero"], fs["tiny"]), (fs["neg"], fs["tiny"])]
    S.count("mps.stereo_gate", 5)


def _mps_accept(S):
    """`if (bestDist <= TH_HIGH)` (:116): 100 is accepted, 101 is not.  A lone candidate has bestDist2 = 256, bestLevel2 = -1."""
    out = []
    for d in (TH_HIGH, TH_HIGH + 1):
        x, y = S.anchor(); B = base_desc()
        q = S.query(x, y, 0, B)
        f = S.feat(x + 1, y, 0, flip(B, d))
        if d == TH_HIGH:
            S.expect[f] = q
        out.append(f)
    S.differ.append(tuple(out))
    S.count("mps.acceptance", 2)


def _mps_ratio(S):
    """`if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;` (:118-121), a float product of a float ratio and an int."""
    nn = F32(S.nnratio)
    prod = F32(nn * F32(50))
    if S.nnratio == 0.9:
        # the exact product 0.9f * 50 = 44.9999988 is below 45, its float32 rounding IS 45.0: `45 > 45.0f` is false and 45 against 50 is ACCEPTED
        # (a double product would reject it); 46 against 50 is rejected
        assert float(nn) * 50 < 45 and prod == F32(45) and not (F32(45) > prod) and F32(46) > prod
        pairs = ((45, 50, True, True), (46, 50, True, False), (46, 50, False, True))
    else:
        assert S.nnratio == 0.8 and float(nn) * 50 > 40 and prod == F32(40)  # exact product above 40, float product 40.0: 40 > 40.0f is false
        pairs = ((40, 50, True, True), (41, 50, True, False), (41, 50, False, True))
    res = []
    for d1, d2, same, ok in pairs:
        x, y = S.anchor(); B = base_desc()
        q = S.query(x, y, 1, B)
        f1 = S.feat(x + 1, y, 1, flip(B, d1)); S.feat(x - 1, y, 1 if same else 0, flip(B, d2, 100))
        if ok:
            S.expect[f1] = q
        res.append((f1, ok))
        S.count("mps.ratio")
    bad = [f for f, ok in res if not ok]
    S.differ += [(f, bad[0]) for f, ok in res if ok]
    # two identical descriptors at distance 0 and one level: 0 > ratio * 0 is false, the first in walk order (one cell, lower index) is matched
    x, y = S.anchor(); B = base_desc(); q = S.query(x, y, 0, B)
    f1 = S.feat(x + 1, y, 0, B); f2 = S.feat(x + 1.5, y, 0, B)
    assert cell(x + 1) == cell(x + 1.5)
    S.expect[f1] = q; S.differ.append((f1, f2))
    # best and runner-up with EQUAL distance 10 at one level: 10 > ratio * 10, rejected
    x, y = S.anchor(); B = base_desc(); S.query(x, y, 0, B)
    f3 = S.feat(x + 1, y, 0, flip(B, 10)); S.feat(x - 1, y, 0, flip(B, 10, 10))
    S.differ.append((f1, f3))
    S.count("mps.ratio", 2)


def _mps_ties(S):
    """Equal distances: `if (dist < bestDist)` is strict (:104-115), so the first in GetFeaturesInArea's walk (cell column, cell row, index) stays best.
    The two candidates are at different levels, so the ratio rule does not reject the tie."""
    lv = 1
    assert S.r(lv) > 4
    layouts = (("column", (3.5, 0.0), (-1.0, 0.0), 1), ("row", (0.0, 3.5), (0.0, -1.0), 1), ("index", (1.0, 0.0), (0.5, 0.0), 0),
               ("column_before_row", (-1.0, 3.5), (3.5, -1.0), 0))
    for name, da, db, winner in layouts:
        x, y = S.anchor(); B = base_desc()
        q = S.query(x, y, lv, B)
        fa = S.feat(x + da[0], y + da[1], lv, flip(B, 10)); fb = S.feat(x + db[0], y + db[1], lv - 1, flip(B, 10, 10))
        ca, cb = (cell(x + da[0]), cell(y + da[1])), (cell(x + db[0]), cell(y + db[1]))
        first = 0 if (ca, fa) < (cb, fb) else 1       # tuple order = (column, row), then index
        assert first == winner, (name, ca, cb)
        if name == "column":
            assert ca[0] > cb[0] and fa < fb          # the lower index lies in the LATER cell
        S.expect[(fa, fb)[winner]] = q
        S.differ.append((fa, fb))
        S.count("mps.ties")


def _mps_order(S):
    """The loop's state (:105-106 `if (F.mvpMapPoints[idx] && Observations() > 0) continue;`, :122-137 the assignment)."""
    # a feature blocked on entry is skipped, and its entry of the in/out table stays
    x, y = S.anchor(); B = base_desc(); q = S.query(x, y, 0, B)
    fb = S.feat(x + 1, y, 0, B, flag=1, init=4321); fo = S.feat(x - 1, y, 0, flip(B, 10))
    S.expect[fo] = q; S.differ.append((fb, fo))
    # two points with observations want one feature: the later one takes its runner-up
    x, y = S.anchor(); B = base_desc()
    q1 = S.query(x, y, 0, B); q2 = S.query(x, y, 0, B)
    fa = S.feat(x + 1, y, 0, B); fr = S.feat(x - 1, y, 0, flip(B, 20))
    S.expect[fa] = q1; S.expect[fr] = q2
    # a point WITHOUT observations blocks nobody: the feature it took is taken again and keeps the later point
    x, y = S.anchor(); B = base_desc()
    S.query(x, y, 0, B, hasObs=0); q4 = S.query(x, y, 0, B)
    fc = S.feat(x + 1, y, 0, B); fn = S.feat(x - 1, y, 0, flip(B, 20))
    S.expect[fc] = q4; S.differ.append((fc, fn))
    # a chain of three: q5 takes fd; q6 finds fd blocked and takes fe (10 against 20: 10 > 0.8 * 20 is false); q7 = fe's descriptor finds fd and fe blocked
    x, y = S.anchor(); B = base_desc()
    fd = S.feat(x + 1, y, 0, B); fe = S.feat(x - 1, y, 0, flip(B, 10)); fg = S.feat(x, y + 1, 0, flip(B, 20))
    q5 = S.query(x, y, 0, B); q6 = S.query(x, y, 0, B); q7 = S.query(x, y, 0, flip(B, 10))
    assert hamming(flip(B, 10), flip(B, 20)) == 10
    S.expect[fd] = q5; S.expect[fe] = q6; S.expect[fg] = q7
    S.count("mps.order_dependence", 4)


def _mps_nan(S):
    """Projections that are NaN or infinite: the reference converts them to int (undefined); required here: no match, no fault."""
    for v in (F32(np.nan), F32(np.inf), F32(-np.inf)):
        B = base_desc()
        S.query(v, 100.0, 0, B); S.query(100.0, v, 0, B)
    S.count("mps.nan_inf", 6)


def mps_problems():
    out = []
    S = MpsScene("mps_th1", "p12", th=1.0, nnratio=0.8, bFar=True, thFar=4.0)
    _mps_window(S, 0); _mps_viewcos(S); _mps_far(S); _mps_dropped(S); _mps_grid_rounding(S); _mps_outside_grid(S); _mps_cell_range(S)
    _mps_levels(S, (0, 2)); _mps_accept(S); _mps_ratio(S); _mps_nan(S)
    out.append(S.problem())
    S = MpsScene("mps_th1_b", "p12", th=1.0, nnratio=0.8, bFar=True, thFar=4.0)
    _mps_stereo(S); _mps_ties(S); _mps_order(S); _mps_levels(S, (7,)); _mps_window(S, 3, exact=False)
    out.append(S.problem())
    S = MpsScene("mps_th3", "p15", th=3.0, nnratio=0.9)
    _mps_window(S, 1); _mps_viewcos(S); _mps_ratio(S); _mps_levels(S, (3,)); _mps_accept(S)
    out.append(S.problem())
    S = MpsScene("mps_p20", "p20", th=1.0, nnratio=0.8)
    _mps_window(S, 2); _mps_levels(S, (0, 1, 2)); _mps_ties(S)
    out.append(S.problem())
    return out


# =========================================================================================================================================
# ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)  (ORBmatcher.cc:1521-1733)
# =========================================================================================================================================
class LastScene(Frame):
    def __init__(self, name, pyr="p12", th=4.0, fwd=0, bwd=0, ori=True):
        super().__init__()
        self.name, self.pyr, self.th, self.fwd, self.bwd, self.ori = name, pyr, th, fwd, bwd, ori
        self.sf = scale_factors(pyr)
        self.last = []

    def r(self, octave):
        return F32(F32(self.th) * self.sf[octave])          # :1585 radius = th * mvScaleFactors[nLastOctave]

    def point(self, X, octave, desc, angle=0.0, valid=1, hasObs=1):
        self.last.append((np.array(X, F32), int(octave), F32(angle), desc, int(valid), int(hasObs)))
        assert len(self.last) <= 128
        return len(self.last) - 1

    def problem(self):
        fa = self.frame_arrays()
        L = self.last
        return dict(entry="last", name=self.name, pyr=self.pyr, th=self.th, fwd=self.fwd, bwd=self.bwd, ori=self.ori, **fa, Tcw=IDENTITY7.copy(),
                    lastK=keypoints([(0.0, 0.0, r[1], r[2]) for r in L]), lastValid=np.array([r[4] for r in L], np.uint8),
                    lastXw=np.stack([r[0] for r in L]).astype(F32), lastDesc=np.stack([r[3] for r in L]).astype(np.uint8),
                    lastObs=np.array([r[5] for r in L], np.uint8), expect=self.expected_table(fa["init"]), differ=list(self.differ),
                    classes=dict(self.classes))


def rotate_identity(q, t, v):
    """Eigen's quaternion * vector as the oracle and q_rotate write it, in float32, then + t."""
    with np.errstate(all="ignore"):
        ux, uy, uz, w = [F32(a) for a in q]
        v = [F32(a) for a in v]
        a = F32(F32(uy * v[2]) - F32(uz * v[1])); b = F32(F32(uz * v[0]) - F32(ux * v[2])); c = F32(F32(ux * v[1]) - F32(uy * v[0]))
        a = F32(a + a); b = F32(b + b); c = F32(c + c)
        o = [F32(F32(v[0] + F32(w * a)) + F32(F32(uy * c) - F32(uz * b))), F32(F32(v[1] + F32(w * b)) + F32(F32(uz * a) - F32(ux * c))),
             F32(F32(v[2] + F32(w * c)) + F32(F32(ux * b) - F32(uy * a)))]
        return [F32(o[i] + F32(t[i])) for i in range(3)]


def _last_minus_zero_reachable():
    """Does any choice of signs for the zero operands (quaternion vector part, translation, v.x, v.y magnitudes 0 / 1) leave x3Dc.z = -0.0?"""
    z = (0.0, -0.0)
    for ux, uy, uz, tz, v0, v1 in itertools.product(z, z, z, z, (0.0, -0.0, 1.0, -1.0), (0.0, -0.0, 1.0, -1.0)):
        o = rotate_identity((ux, uy, uz, 1.0), (0.0, 0.0, tz), (v0, v1, -0.0))
        if o[2] == 0 and np.signbit(o[2]):
            return True
    return False


def last_main():
    S = LastScene("last_main", "p12", th=4.0)
    tiny = np.finfo(F32).tiny
    assert not _last_minus_zero_reachable()
    # -- depth sign (:1563-1566 `invzc = 1.0 / x3Dc(2); if (invzc < 0) continue;`): a tiny positive depth is searched at the principal point, a negative one
    # is not; z = +0.0 on the axis projects to NaN, which passes both bounds tests and must match nothing
    B = base_desc(); q = S.point((0.0, 0.0, tiny), 0, B); f = S.feat(CX + 1, CY, 0, flip(B, 10)); S.expect[f] = q
    B2 = base_desc(); S.point((0.0, 0.0, -tiny), 0, B2); S.point((0.0, 0.0, -1.0), 0, B2); f2 = S.feat(CX - 40, CY, 0, B2)
    B3 = base_desc(); S.point((0.0, 0.0, 0.0), 0, B3); S.point((1.0, 0.0, 0.0), 0, B3); S.point((-1.0, 0.0, -0.0), 0, B3); S.feat(CX + 40, CY, 0, B3)
    S.differ.append((f, f2))
    S.count("last.depth_sign", 6)
    # -- image bounds (:1571-1574), closed: u == maxX is searched (its window reaches the last grid column), one ulp outside is not
    lv = 2
    r = S.r(lv)
    assert r > 5.5
    ulp0 = F32(-2.0 ** -15)
    u_of = lambda a: F32(F32(F32(FX) * F32(a)) / F32(1.0)) + F32(CX)
    v_of = lambda a: F32(F32(F32(FY) * F32(a)) / F32(1.0)) + F32(CY)
    for axis, fn, lo, hi, c in ((0, u_of, 0.0, 512.0, CX), (1, v_of, 0.0, 384.0, CY)):
        for target, start, fpos, ok in ((F32(hi), (hi - c) / 256, hi - 5, True), (up(hi), (hi - c) / 256, hi - 5, False),
                                        (F32(lo), (lo - c) / 256, lo + 1, True), (ulp0, (lo - c) / 256, lo + 1, False)):
            a = solve(fn, target, start)
            B = base_desc()
            other = F32((42, 90, 138, 282, 58, 114, 170, 338)[S.classes.get("last.bounds", 0)])      # a row / column of its own
            q = S.point((a, F32(F32(other - F32(CY)) / F32(FY)), 1.0) if axis == 0 else (F32(F32(other - F32(CX)) / F32(FX)), a, 1.0), lv, B)
            f = S.feat(fpos, other, lv, flip(B, 10)) if axis == 0 else S.feat(other, fpos, lv, flip(B, 10))
            assert 0 <= cell(fpos) < (64 if axis == 0 else 48)
            if ok:
                S.expect[f] = q; good = f
            else:
                S.differ.append((good, f))
            S.count("last.bounds")
    return S.problem()


def _pair(S, octave, fo, B, d, z=1.0, angle_last=0.0, angle_cur=0.0, ur=-1.0, hasObs=1, flag=0):
    """One last-frame point at its own anchor with one current feature 1 px beside its projection."""
    x, y = S.anchor()
    q = S.point(backproject(x, y, z), octave, B, angle=angle_last, hasObs=hasObs)
    f = S.feat(x + 1, y, fo, flip(B, d), ur=ur, angle=angle_cur, flag=flag)
    return q, f, (x, y)


def last_levels(fwd, bwd):
    """:1590-1600: bForward GetFeaturesInArea(.., nLastOctave) (minLevel only; at octave 0 no level is checked at all), else bBackward (0, nLastOctave), else
    (nLastOctave - 1, nLastOctave + 1).  Written out as a table per mode; with both flags set the forward branch is taken."""
    S = LastScene("last_levels_f%d_b%d" % (fwd, bwd), "p12", th=4.0, fwd=fwd, bwd=bwd)
    allowed = (lambda o, fo: fo >= o) if fwd else (lambda o, fo: fo <= o) if bwd else (lambda o, fo: abs(fo - o) <= 1)
    for n, o in enumerate((0, 7, 3)):
        ins, outs = [], []
        for fo in range(max(0, o - 2), min(7, o + 2) + 1):
            q, f, _ = _pair(S, o, fo, base_desc(), 10, z=(1.0, 2.0, 4.0)[n])
            if allowed(o, fo):
                S.expect[f] = q; ins.append(f)
            else:
                outs.append(f)
            S.count("last.level_range")
        S.differ += [(ins[0], x) for x in outs]
    # -- acceptance `if (bestDist <= TH_HIGH)` (:1617)
    q, f, _ = _pair(S, 0, 0, base_desc(), TH_HIGH); S.expect[f] = q
    _, f2, _ = _pair(S, 0, 0, base_desc(), TH_HIGH + 1)
    S.differ.append((f, f2))
    S.count("last.acceptance", 2)
    # -- stereo gate (:1605-1611): ur = u - mbf * invzc, `if (er > radius) continue;`, only for mvuRight > 0
    r = S.r(0)
    fs = {}
    for name, off in (("kept", r), ("gone", None), ("zero", None)):
        x, y = S.anchor(); B = base_desc()
        q = S.point(backproject(x, y, 2.0), 0, B)
        xr = F32(x - F32(F32(MBF) * F32(0.5)))
        ur = {"kept": F32(xr + r), "gone": up(F32(xr + r)), "zero": F32(0.0)}[name]
        assert (name != "kept" or abs(F32(xr - ur)) == r) and (name != "gone" or abs(F32(xr - ur)) > r)
        fs[name] = S.feat(x + 1, y, 0, flip(B, 10), ur=ur)
        if name != "gone":
            S.expect[fs[name]] = q
    S.differ += [(fs["kept"], fs["gone"]), (fs["zero"], fs["gone"])]
    S.count("last.stereo_gate", 3)
    return S.problem()


def _histogram(S, bins, pair):
    """Accepted matches by count: `bins` = [(rot in degrees, how many, kept)]; pair(rot) adds one match whose angle difference is rot and returns
    (query row, output row).  Returns the output rows per bin."""
    rows = []
    for rot, n, kept in bins:
        rs = []
        for _ in range(n):
            q, f = pair(rot)
            if kept:
                S.expect[f] = q
            rs.append(f)
        rows.append(rs)
    return rows


# the histogram edges every copy of ComputeThreeMaxima (ORBmatcher.cc:1844-1876) is run through: name -> [(rot, count, kept)]
HISTOGRAMS = {
    # four equal bins: `s > max1`, `s > max2`, `s > max3` are strict, so the first three in bin order stay and the fourth is removed
    "equal_maxima": [(60, 3, True), (120, 3, True), (210, 3, True), (330, 3, False)],
    # (10, 1): max2 < 0.1f * max1 is 1 < 1.0f, false: the second bin is kept
    "ten_one": [(120, 10, True), (270, 1, True)],
    # (20, 1, 1): 1 < 2.0f: the second and third bins are dropped
    "twenty_one": [(120, 20, True), (270, 1, False), (30, 1, False)],
    # the same two edges on the third bin: (10, 5, 1) keeps it, (20, 5, 1) drops it
    "third_ten": [(120, 10, True), (270, 5, True), (30, 1, True)],
    "third_twenty": [(120, 20, True), (270, 5, True), (30, 1, False)],
    "one_bin": [(90, 4, True)],
    "two_bins": [(90, 4, True), (300, 2, True)],
}
assert F32(F32(0.1) * F32(10)) == F32(1.0) and F32(F32(0.1) * F32(20)) == F32(2.0)     # 0.1f * (float)max1 at the two edges


def _check_histogram(bins):
    """Every row of a histogram falls into a bin of its own (through rot_bin(), the kernel's arithmetic): the counts are what the table says."""
    hist = {}
    for rot, n, _ in bins:
        assert rot_bin(rot) not in hist and 0 <= rot_bin(rot) <= 12, "two rows share a bin"
        hist[rot_bin(rot)] = n
    return hist


def last_histogram(name, fwd=0):
    S = LastScene("last_hist_" + name, "p12", th=4.0, fwd=fwd)
    _check_histogram(HISTOGRAMS[name])

    def pair(rot):
        q, f, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=F32(rot), angle_cur=0.0)
        return q, f
    rows = _histogram(S, HISTOGRAMS[name], pair)
    kept = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and b[2]]; gone = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and not b[2]]
    S.differ += [(kept[0], g) for g in gone]
    S.count("last.rotation_histogram")
    return S.problem()


def last_rotation_bins():
    """The bin of one match (:1625-1632): rot == 0, rot < 0 (360 is added), and rot * (1.0f / 30) == 0.5 exactly (rot = 15), which round() sends to
    bin 1.  Bin 1 holds 20 matches of rot 30 / -330 and the rot-15 one, bin 0 the rot-0 one: 1 < 0.1f * 21, so the rot-0 match is removed and the
    rot-15 one stays.  With round-half-even the counts would be (20, 2) and both would stay."""
    S = LastScene("last_rotation_bins", "p12", th=4.0)
    assert F32(F32(15.0) * F32(F32(1.0) / F32(30))) == F32(0.5) and rot_bin(15.0) == 1 and rot_bin(0.0) == 0
    assert F32(F32(10.0) - F32(340.0)) < 0 and rot_bin(F32(F32(10.0) - F32(340.0))) == 1 and rot_bin(30.0) == 1
    for i in range(20):
        if i % 2:
            q, f, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=10.0, angle_cur=340.0)     # rot = -330 -> 30
        else:
            q, f, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=40.0, angle_cur=10.0)
        S.expect[f] = q
    q, f15, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=25.0, angle_cur=10.0)
    S.expect[f15] = q
    _, f0, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=77.0, angle_cur=77.0)
    S.differ.append((f15, f0))
    S.count("last.rotation_bins", 4)
    return S.problem()


def last_claimed_twice():
    """A feature claimed by two queries (the first point has no observations, so it does not block) whose EARLIER entry lies in a removed bin: the filter
    walks every entry of the removed bins and clears CurrentFrame.mvpMapPoints[rotHist[i][j]] (:1722-1728), so the later, surviving claim is cleared too.
    Bins: 120 degrees x 20 (kept), 270 degrees x 1 = the earlier claim (1 < 2.0f: removed)."""
    S = LastScene("last_claimed_twice", "p12", th=4.0)
    for _ in range(19):
        q, f, _ = _pair(S, 0, 0, base_desc(), 10, angle_last=120.0)
        S.expect[f] = q
    x, y = S.anchor(); B = base_desc()
    S.point(backproject(x, y, 1.0), 0, B, angle=270.0, hasObs=0)
    S.point(backproject(x, y, 1.0), 0, B, angle=120.0)
    fc = S.feat(x + 1, y, 0, B, init=777)
    S.expect[fc] = -1
    S.differ.append((0, fc))
    S.count("last.rotation_claimed_twice")
    return S.problem()


def last_order():
    """blocked on entry (:1601-1603 `if (CurrentFrame.mvpMapPoints[i2]) if (Observations() > 0) continue;`), and the later of two claims wins."""
    S = LastScene("last_order", "p20", th=4.0, ori=False)
    x, y = S.anchor(); B = base_desc(); q = S.point(backproject(x, y, 4.0), 0, B)
    fb = S.feat(x + 1, y, 0, B, flag=1, init=99); fo = S.feat(x - 1, y, 0, flip(B, 30)); S.expect[fo] = q; S.differ.append((fb, fo))
    x, y = S.anchor(); B = base_desc(); q1 = S.point(backproject(x, y, 2.0), 0, B); q2 = S.point(backproject(x, y, 2.0), 0, B)
    fa = S.feat(x + 1, y, 0, B); fr = S.feat(x - 1, y, 0, flip(B, 30)); S.expect[fa] = q1; S.expect[fr] = q2
    x, y = S.anchor(); B = base_desc(); S.point(backproject(x, y, 2.0), 1, B, hasObs=0); q4 = S.point(backproject(x, y, 2.0), 1, B)
    fc = S.feat(x + 1, y, 1, B); S.expect[fc] = q4
    # top octave of this pyramid, window edge |dx| == r = 4 * 4 exactly
    x, y = S.anchor(); B = base_desc(); q = S.point(backproject(x, y, 1.0), 2, B); r = S.r(2)
    assert r == 16 and F32(F32(x + r) - x) == r
    fe = S.feat(x + r, y, 2, B); fi = S.feat(dn(x + r), y, 2, flip(B, 10)); S.expect[fi] = q; S.differ.append((fe, fi))
    S.count("last.order_dependence", 3); S.count("last.window", 1)
    return S.problem()


def last_problems():
    return ([last_main()] + [last_levels(f, b) for f, b in ((0, 0), (1, 0), (0, 1), (1, 1))] + [last_histogram(n) for n in HISTOGRAMS] +
            [last_rotation_bins(), last_claimed_twice(), last_order()])


# =========================================================================================================================================
# SearchByProjection(CurrentFrame, KeyFrame, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1735-1842)
# =========================================================================================================================================
def kf_problems():
    """`if (bestDist <= ORBdist)` (:1805) at ORBdist and ORBdist + 1, a current feature that already holds a map point (:1794-1795), the two distance
    bounds (:1769-1774), and one histogram edge through the same filter."""
    out = []
    for name, orb, bins in (("kf_orb60", 60, None), ("kf_hist_ten_one", 100, HISTOGRAMS["ten_one"]), ("kf_hist_twenty_one", 100, HISTOGRAMS["twenty_one"])):
        S = LastScene(name, "p12", th=4.0)
        pts = []

        def pair(d, rot=0.0, maxD=None, minD=0.0, flag=0, init=-1):
            x, y = S.anchor(); B = base_desc()
            X = backproject(x, y, 2.0)
            dist = np.sqrt(F32(F32(F32(X[0] * X[0]) + F32(X[1] * X[1])) + F32(X[2] * X[2])))
            q = S.point(X, 0, B, angle=F32(rot))
            pts.append((F32(dist) if maxD is None else maxD(dist), minD if not callable(minD) else minD(dist)))   # maxD = dist: ratio 1, level 0
            f = S.feat(x + 1, y, 0, flip(B, d), flag=flag, init=init)
            return q, f
        if bins is None:
            q, f = pair(orb); S.expect[f] = q
            _, f2 = pair(orb + 1); S.differ.append((f, f2)); S.count("kf.acceptance", 2)
            _, f3 = pair(5, flag=1, init=31); S.differ.append((f, f3)); S.count("kf.has_map_point")
            mx = lambda m: F32(F32(1.2) * F32(m)); mn = lambda m: F32(F32(0.8) * F32(m))
            q, f4 = pair(5, maxD=lambda d_: solve(mx, d_, d_ / 1.2)); S.expect[f4] = q
            _, f5 = pair(5, maxD=lambda d_: solve(mx, dn(d_), d_ / 1.2)); S.differ.append((f4, f5))
            q, f6 = pair(5, minD=lambda d_: solve(mn, d_, d_ / 0.8)); S.expect[f6] = q
            _, f7 = pair(5, minD=lambda d_: solve(mn, up(d_), d_ / 0.8)); S.differ.append((f6, f7))
            S.count("kf.distance", 4)
        else:
            _check_histogram(bins)
            rows = _histogram(S, bins, lambda rot: pair(10, rot))
            kept = [r[0] for r, b in zip(rows, bins) if r and b[2]]; gone = [r[0] for r, b in zip(rows, bins) if r and not b[2]]
            S.differ += [(kept[0], g) for g in gone] if gone else []
            S.count("kf.rotation_histogram")
        p = S.problem()
        p.update(entry="kf", orb=orb, Ow=np.zeros(3, F32), maxD=np.array([a for a, _ in pts], F32), minD=np.array([b for _, b in pts], F32))
        out.append(p)
    return out


# =========================================================================================================================================
# The keyframe projections: Fuse (ORBmatcher.cc:1044-1213 and :1215-1321), SearchByProjection(KF, Scw) (:397-494), SearchBySim3 (:1323-1519)
# =========================================================================================================================================
class KfScene(Frame):
    """Map points projected into a keyframe with the identity pose (Ow = 0); one predicted level per point through maxDist = dist * ratio."""

    def __init__(self, name, pyr="p12", th=6.0):
        super().__init__()
        self.name, self.pyr, self.th = name, pyr, th
        self.sf = scale_factors(pyr)
        self.pts = []
        self.expect_by = {}          # entry -> {point row: feature}: where the entries differ

    def mp(self, X, desc, maxD=None, minD=0.0, normal=None, valid=1):
        X = np.array(X, F32)
        d = np.sqrt(F32(F32(F32(X[0] * X[0]) + F32(X[1] * X[1])) + F32(X[2] * X[2])))
        self.pts.append((X, desc, F32(d if maxD is None else maxD), F32(minD), np.array(X if normal is None else normal, F32), int(valid)))
        assert len(self.pts) <= 128
        return len(self.pts) - 1

    def problem(self, entry, by_feature=False, **kw):
        """expect[point] = feature; by_feature: expect[feature] = point (SearchByProjection(KF, Scw) fills a feature-indexed table)."""
        fa = self.frame_arrays()
        P = self.pts
        n = len(P)
        e = np.full(len(fa["k"]) if by_feature else n, -1, np.int32)
        for i, f in {**self.expect, **self.expect_by.get(entry, {})}.items():
            e[i] = f
        return dict(entry=entry, name=self.name + "_" + entry, pyr=self.pyr, th=self.th, **fa, Tcw=IDENTITY7.copy(), Ow=np.zeros(3, F32),
                    valid=np.array([p[5] for p in P], np.uint8), Pw=np.stack([p[0] for p in P]), normal=np.stack([p[4] for p in P]),
                    maxD=np.array([p[2] for p in P], F32), minD=np.array([p[3] for p in P], F32), mpDesc=np.stack([p[1] for p in P]).astype(np.uint8),
                    expect=e, differ=list(self.differ), classes=dict(self.classes), **kw)


def kfproj_scene():
    """One keyframe and its map points for Fuse (both forms) and SearchByProjection(KF, Scw): expect[point] = feature.  Every feature lies 1 px from its
    projection at level 0, inside Fuse's chi-square gate (1 < 5.99)."""
    S = KfScene("kfproj", "p12", th=6.0)

    def one(X, d=10, fo=0, dx=1.0, **kw):
        B = base_desc()
        u = F32(F32(F32(FX) * F32(X[0])) / F32(X[2])) + F32(CX); v = F32(F32(F32(FY) * F32(X[1])) / F32(X[2])) + F32(CY)
        i = S.mp(X, B, **kw)
        f = S.feat(u + dx, v, fo, flip(B, d))
        return i, f
    # -- KeyFrame::IsInImage (KeyFrame.cc:776-779), half open: u == minX is kept, u == maxX is dropped; the same for v
    u_of = lambda a: F32(F32(F32(FX) * F32(a)) / F32(1.0)) + F32(CX)
    v_of = lambda a: F32(F32(F32(FY) * F32(a)) / F32(1.0)) + F32(CY)
    for axis, fn, hi, c in ((0, u_of, 512.0, CX), (1, v_of, 384.0, CY)):
        row = F32(66 + 48 * len(S.pts))
        mk = lambda a: (a, F32(F32(row - F32(CY)) / F32(FY)), 1.0) if axis == 0 else (F32(F32(row - F32(CX)) / F32(FX)), a, 1.0)
        res = {}
        for name, target, start in (("min", F32(0.0), -c / 256), ("max", F32(hi), (hi - c) / 256), ("below_max", dn(hi), (hi - c) / 256)):
            a = solve(fn, target, start)
            B = base_desc()
            i = S.mp(mk(a), B)
            fpos = 1.0 if name == "min" else hi - 5
            f = S.feat(fpos, row, 0, flip(B, 10)) if axis == 0 else S.feat(row, fpos, 0, flip(B, 10))
            res[name] = (i, f)
            row = F32(row + 48)
        S.expect_by.setdefault("fuse_sim3", {}).update({res[k][0]: res[k][1] for k in ("min", "below_max")})
        S.expect_by.setdefault("sim3", {}).update({res[k][0]: res[k][1] for k in ("min", "below_max")})
        S.expect_by.setdefault("fuse", {}).update({res["min"][0]: res["min"][1]})     # below_max: 5 px away, 25 > 5.99: the gate rejects it in Fuse
        S.differ += [(res["min"][0], res["max"][0])]
        S.count("kfproj.is_in_image", 3)
    # -- depth sign (:1115-1116 `if (p3Dc(2) < 0.0f) continue;`): negative is dropped; zero divides (infinite / NaN projection): no match required
    x, y = S.anchor()
    i, f = one(backproject(x, y, 1.0)); S.expect[i] = f
    B = base_desc(); j = S.mp(-backproject(x + 8, y, 1.0), B); S.feat(x + 9, y, 0, B)
    B = base_desc(); S.mp((0.0, 0.0, 0.0), B); S.mp((1.0, 0.0, 0.0), B)
    S.differ.append((i, j)); S.count("kfproj.depth_sign", 4)
    # -- distance bounds (:1133-1137) and the normal test (:1139-1143 `if (PO.dot(Pn) < 0.5 * dist3D) continue;`, a double comparison)
    mx = lambda m: F32(F32(1.2) * F32(m)); mn = lambda m: F32(F32(0.8) * F32(m))
    X = np.array([0.0, 0.0, 2.0], F32)                 # dist3D = 2 exactly
    for kw, ok in ((dict(maxD=solve(mx, F32(2.0), 2 / 1.2)), True), (dict(maxD=solve(mx, dn(2.0), 2 / 1.2)), False),
                   (dict(maxD=2.0, minD=solve(mn, F32(2.0), 2.5)), True), (dict(maxD=2.0, minD=solve(mn, up(2.0), 2.5)), False),
                   (dict(maxD=2.0, normal=(0.0, 0.0, 0.5)), True), (dict(maxD=2.0, normal=(0.0, 0.0, dn(0.5))), False)):
        # all six project to the principal point: each gets its own feature through its own descriptor, 60 bits from every other
        B = base_desc()
        i = S.mp(X, B, **kw)
        if ok:
            good = i
        else:
            S.differ.append((good, i))
        S._axis = getattr(S, "_axis", []) + [(i, B, ok)]
    assert F32(F32(2.0) * F32(0.5)) == 1.0 and float(F32(F32(2.0) * dn(0.5))) < 0.5 * 2.0
    for n, (i, B, ok) in enumerate(S._axis):
        f = S.feat(CX + 1, F32(CY - 1.25 + 0.5 * n), 0, flip(B, 10))     # e2 <= 1 + 1.25^2: inside Fuse's gate
        if ok:
            S.expect[i] = f
    S.count("kfproj.distance", 4); S.count("kfproj.normal", 2)
    # -- acceptance `if (bestDist <= TH_LOW)` (:1190, :1303): 50 and 51
    x, y = S.anchor(); i, f = one(backproject(x, y, 2.0), d=TH_LOW); S.expect[i] = f
    x, y = S.anchor(); j, _ = one(backproject(x, y, 2.0), d=TH_LOW + 1)
    S.differ.append((i, j)); S.count("kfproj.acceptance", 2)
    # -- level filter (:1149-1150 `if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;`) at predicted level 0 and 2
    for ratio, lv in ((1.0, 0), (1.3, 2)):
        for fo in range(max(0, lv - 2), lv + 2):
            x, y = S.anchor(); X = backproject(x, y, 1.0)
            d3 = np.sqrt(F32(F32(F32(X[0] * X[0]) + F32(X[1] * X[1])) + F32(X[2] * X[2])))
            i, f = one(X, fo=fo, maxD=F32(d3 * F32(ratio)))
            if fo in (lv - 1, lv):
                S.expect[i] = f; inside = i
            else:
                S.differ.append((inside, i)) if fo > lv else None
            S.count("kfproj.levels")
    return S


def _e2_inputs(target, stereo):
    """Feature coordinates around the projection (8, 8) whose float32 e2 equals `target` exactly.  Near the origin the keypoint spacing is 2^-21 or
    less, fine enough that scanning one coordinate reaches every float32 in [4, 8).  mono: ex = 2.4375 fixed, ey scanned (e2 = ex * ex + ey * ey);
    stereo: ex = 2, ey = 0, xr = 0 and uRight scanned (e2 = ex * ex + ey * ey + er * er with er = xr - uRight)."""
    u = v = F32(8.0)
    if not stereo:
        fx_ = F32(8.0 - 2.4375)
        e2 = lambda fy_: F32(F32(F32(u - fx_) * F32(u - fx_)) + F32(F32(v - F32(fy_)) * F32(v - F32(fy_))))
        fy_ = solve(e2, target, 8.0 - np.sqrt(float(target) - 2.4375 ** 2), steps=4096)
        return fx_, fy_, F32(-1.0), e2(fy_)
    e2 = lambda ur: F32(F32(F32(F32(2.0) * F32(2.0)) + F32(F32(0.0) * F32(0.0))) + F32(F32(F32(0.0) - F32(ur)) * F32(F32(0.0) - F32(ur))))
    ur = solve(e2, target, np.sqrt(float(target) - 4.0), steps=4096)
    return F32(6.0), v, ur, e2(ur)


def fuse_gate_scenes():
    """Fuse's reprojection gate (:1160-1181): e2 * mvInvLevelSigma2[level] > 5.99 (mono) or > 7.8 (stereo) rejects, both compared in double.  5.99 and 7.8
    are not float32 values, so the two float32 neighbours of each bound are used, one tiny frame each: a point at depth 4 that projects to (8, 8) with
    xr = 8 - 32 / 4 = 0, and one level-0 feature (invSigma2 = 1) placed by _e2_inputs.  uRight == 0 takes the STEREO branch (`mvuRight[idx] >= 0`),
    uRight == -1 the mono one."""
    lo599 = F32(5.99) if float(F32(5.99)) <= 5.99 else dn(5.99); hi599 = up(lo599)
    lo78 = F32(7.8) if float(F32(7.8)) <= 7.8 else dn(7.8); hi78 = up(lo78)
    assert float(lo599) <= 5.99 < float(hi599) and float(lo78) <= 7.8 < float(hi78)
    out = []
    for name, target, stereo, bound in (("mono_lo", lo599, False, 5.99), ("mono_hi", hi599, False, 5.99), ("stereo_lo", lo78, True, 7.8),
                                        ("stereo_hi", hi78, True, 7.8)):
        S = KfScene("fuse_gate_" + name, "p12", th=6.0)
        B = base_desc()
        X = backproject(8.0, 8.0, 4.0)
        assert F32(F32(8.0) - F32(F32(MBF) * F32(F32(1.0) / X[2]))) == 0          # ur = u - mbf * invz (:1125)
        i = S.mp(X, B)
        fx_, fy_, ur, e2 = _e2_inputs(target, stereo)
        f = S.feat(fx_, fy_, 0, flip(B, 10), ur=ur)
        ok = not (float(F32(e2 * F32(F32(1.0) / F32(1.0)))) > bound)
        assert e2 == target and ok == name.endswith("lo")
        if ok:
            S.expect[i] = f
        S.count("fuse.chi2_gate")
        out.append(S)
    # uRight == 0: the stereo branch.  ex = 2 and er = xr - 0 = x - 16 is large: e2 > 7.8, rejected; with uRight == -1 the same feature passes the mono
    # gate (4 < 5.99)
    S = KfScene("fuse_gate_uright", "p12", th=6.0)
    res = []
    for ur in (0.0, -1.0):
        x, y = S.anchor(); B = base_desc()
        i = S.mp(backproject(x, y, 2.0), B); f = S.feat(x - 2, y, 0, flip(B, 10), ur=ur)
        if ur < 0:
            S.expect[i] = f
        res.append(i)
    S.differ.append((res[1], res[0]))
    S.count("fuse.uright_zero", 2)
    out.append(S)
    return out


def kfproj_problems():
    out = []
    S = kfproj_scene()
    out.append(S.problem("fuse", sim3Form=False))
    out.append(S.problem("fuse_sim3", sim3Form=True))
    out += [G.problem("fuse", sim3Form=False) for G in fuse_gate_scenes()]
    return out


def sim3_problems():
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (:397-494): `if (bestDist <= TH_LOW * ratioHamming)` compares an int with the
    float product of an int and a float.  0.9f is 0.899999976 and the exact product 44.9999988 is below 45, but its float32 rounding is 45.0: the
    threshold with 0.9 is 45 in the reference's arithmetic (a double product would make it 44).
    The table is indexed by FEATURE here: expect[feature] = point."""
    out = []
    for ratio in (1.0, 0.9):
        S = KfScene("sim3_r%02d" % int(ratio * 10), "p12", th=6)
        lim = F32(F32(TH_LOW) * F32(ratio))
        top = TH_LOW if ratio == 1.0 else 45
        assert F32(top) <= lim < F32(top + 1) and (ratio == 1.0 or (lim == F32(45) and float(F32(ratio)) * TH_LOW < 45))
        res = []
        for d in (top, top + 1):
            x, y = S.anchor(); B = base_desc()
            i = S.mp(backproject(x, y, 2.0), B); f = S.feat(x + 1, y, 0, flip(B, d))
            if d == top:
                S.expect[f] = i
            res.append(f)
        S.differ.append(tuple(res))
        # a feature matched on entry is skipped (:468-469); the point takes the other one
        x, y = S.anchor(); B = base_desc()
        i = S.mp(backproject(x, y, 2.0), B); fm = S.feat(x + 1, y, 0, B, flag=1); fo = S.feat(x - 1, y, 0, flip(B, 10))
        S.expect[fo] = i; S.differ.append((fm, fo))
        # two points want one feature: vpMatched[bestIdx] is set by the first (:483), the second takes its runner-up
        x, y = S.anchor(); B = base_desc()
        i1 = S.mp(backproject(x, y, 2.0), B); i2 = S.mp(backproject(x, y, 2.0), B)
        fa = S.feat(x + 1, y, 0, B); fr = S.feat(x - 1, y, 0, flip(B, 10)); S.expect[fa] = i1; S.expect[fr] = i2
        S.count("sim3.acceptance", 2); S.count("sim3.matched", 2)
        out.append(S.problem("sim3", by_feature=True, ratio=ratio, manual=False))
    return out


def sim3dir_problem():
    """SearchBySim3 (:1323-1519) between two keyframes with identity poses and S12 = S21 = identity: each keyframe's points are searched in the other;
    match12[i1] = idx2 only where vnMatch1[i1] == idx2 and vnMatch2[idx2] == i1 (:1501-1516).  Points are rows of the keyframe's own feature table."""
    A, Bf = KfScene("sim3dir_A", "p12", th=6.0), KfScene("sim3dir_B", "p12", th=6.0)
    ptsA, ptsB = {}, {}        # feature row -> (X, desc)

    def add(scene, x, y, desc, fo=0):
        return scene.feat(x, y, fo, desc)
    e1, e2, e12 = {}, {}, {}
    # mutual: A's feature a at (x, y) owns a point that projects onto B's feature b 1 px aside, and the other way round
    x, y = A.anchor(); Bf.anchor(); D = base_desc()
    a = add(A, x, y, D); b = add(Bf, x + 1, y, flip(D, 5)); ptsA[a] = (backproject(x + 1, y, 2.0), D); ptsB[b] = (backproject(x, y, 2.0), flip(D, 5))
    e1[a] = b; e2[b] = a; e12[a] = b
    # one-sided: B's feature b2 has no point, so nothing points back at a2
    x, y = A.anchor(); Bf.anchor(); D = base_desc()
    a2 = add(A, x, y, D); b2 = add(Bf, x + 1, y, flip(D, 5)); ptsA[a2] = (backproject(x + 1, y, 2.0), D)
    e1[a2] = b2
    # disagreement: b3's point lands on another feature of A (a4) although a3's point lands on b3
    x, y = A.anchor(); Bf.anchor(); D = base_desc(); E = base_desc()
    a3 = add(A, x, y, D); b3 = add(Bf, x + 1, y, flip(D, 5)); a4 = add(A, x + 20, y, E)
    ptsA[a3] = (backproject(x + 1, y, 2.0), D); ptsB[b3] = (backproject(x + 20, y, 2.0), E)
    e1[a3] = b3; e2[b3] = a4
    # acceptance `if (bestDist <= TH_HIGH)` (:1416): 100 and 101
    for d, ok in ((TH_HIGH, True), (TH_HIGH + 1, False)):
        x, y = A.anchor(); Bf.anchor(); D = base_desc()
        a5 = add(A, x, y, D); b5 = add(Bf, x + 1, y, flip(D, d)); ptsA[a5] = (backproject(x + 1, y, 2.0), D)
        if ok:
            e1[a5] = b5; good = a5
        else:
            A.differ.append((good, a5))
    # vnMatch1 pointing past keyframe A's count: B has MORE features than A; A's point matches B's last feature, whose index is beyond A's count
    while len(Bf.rows) <= len(A.rows) + 3:
        Bf.feat(470.0, F32(20 + 6 * len(Bf.rows)), 3, base_desc())
    x, y = A.anchor(); D = base_desc()
    a6 = add(A, x, y, D); b6 = add(Bf, x + 1, y, flip(D, 5)); ptsA[a6] = (backproject(x + 1, y, 2.0), D)
    assert b6 >= len(A.rows)
    e1[a6] = b6
    A.count("sim3dir.agreement", 4); A.count("sim3dir.acceptance", 2)
    fa, fb = A.frame_arrays(), Bf.frame_arrays()

    def tables(n, pts):
        v = np.zeros(n, np.uint8); X = np.zeros((n, 3), F32); D = np.zeros((n, 32), np.uint8); mx = np.ones(n, F32)
        for i, (x3, d) in pts.items():
            v[i] = 1; X[i] = x3; D[i] = d
            mx[i] = np.sqrt(F32(F32(F32(x3[0] * x3[0]) + F32(x3[1] * x3[1])) + F32(x3[2] * x3[2])))
        return dict(valid=v, Pw=X, mpDesc=D, maxD=mx, minD=np.zeros(n, F32))
    nA, nB = len(fa["k"]), len(fb["k"])
    ex = lambda n, e: np.array([e.get(i, -1) for i in range(n)], np.int32)
    return dict(entry="sim3dir", name="sim3dir", pyr="p12", th=6.0, A=fa, B=fb, ptsA=tables(nA, ptsA), ptsB=tables(nB, ptsB),
                S=np.array([0, 0, 0, 1, 0, 0, 0, 0], F32)[:7], expect1=ex(nA, e1), expect2=ex(nB, e2), expect12=ex(nA, e12),
                differ=list(A.differ), classes=dict(A.classes))


# =========================================================================================================================================
# ORBmatcher::SearchForInitialization (ORBmatcher.cc:603-700)
# =========================================================================================================================================
class InitScene(Frame):
    """Frame = F2; F1's features are the queries, searched around vbPrevMatched (here: their own position) with r = windowSize."""

    def __init__(self, name, nnratio=0.8, win=10, ori=True):
        super().__init__()
        self.name, self.nnratio, self.win, self.ori = name, nnratio, win, ori
        self.f1 = []

    def q(self, x, y, octave, desc, angle=0.0):
        self.f1.append((F32(x), F32(y), int(octave), F32(angle), desc))
        assert len(self.f1) <= 128
        return len(self.f1) - 1

    def problem(self):
        fa = self.frame_arrays()
        n1 = len(self.f1)
        e = np.full(n1, -1, np.int32)
        for i, f in self.expect.items():
            e[i] = f
        return dict(entry="init", name=self.name, pyr="p12", nnratio=self.nnratio, win=self.win, ori=self.ori, k2=fa["k"], d2=fa["d"],
                    k1=keypoints([r[:4] for r in self.f1]), d1=np.stack([r[4] for r in self.f1]).astype(np.uint8),
                    prev=np.array([[r[0], r[1]] for r in self.f1], F32), expect=e, differ=list(self.differ), classes=dict(self.classes))


def init_main(nnratio):
    S = InitScene("init_r%02d" % int(nnratio * 10), nnratio=nnratio)
    # -- octave (:620-622 `if (level1 > 0) continue;`), and F2 features above octave 0 are no candidates (GetFeaturesInArea(.., level1, level1))
    x, y = S.anchor(); B = base_desc(); i0 = S.q(x, y, 0, B); f = S.feat(x + 1, y, 0, flip(B, 10)); S.expect[i0] = f
    x, y = S.anchor(); B = base_desc(); i1 = S.q(x, y, 1, B); S.feat(x + 1, y, 0, flip(B, 10))
    x, y = S.anchor(); B = base_desc(); i2 = S.q(x, y, 0, B); S.feat(x + 1, y, 1, flip(B, 10))
    S.differ += [(i0, i1), (i0, i2)]; S.count("init.octave", 3)
    # -- acceptance `if (bestDist <= TH_LOW)` (:645)
    x, y = S.anchor(); B = base_desc(); a = S.q(x, y, 0, B); f = S.feat(x + 1, y, 0, flip(B, TH_LOW)); S.expect[a] = f
    x, y = S.anchor(); B = base_desc(); b = S.q(x, y, 0, B); S.feat(x + 1, y, 0, flip(B, TH_LOW + 1))
    S.differ.append((a, b)); S.count("init.acceptance", 2)
    # -- ratio `if (bestDist < (float)bestDist2 * mfNNratio)` (:647), strict, a float product
    nn = F32(nnratio)
    prod = F32(F32(50) * nn)
    if nnratio == 0.8:
        assert prod == F32(40) and float(nn) * 50 > 40          # float: 40 < 40.0f is false (rejected); exact arithmetic would accept
        pairs = ((40, False), (39, True))
    else:
        assert nnratio == 0.9 and prod == F32(45) and F32(44) < prod  # 45 < 45.0f is false, 44 passes
        pairs = ((45, False), (44, True))
    res = []
    for d1, ok in pairs:
        x, y = S.anchor(); B = base_desc(); i = S.q(x, y, 0, B)
        f = S.feat(x + 1, y, 0, flip(B, d1)); S.feat(x - 1, y, 0, flip(B, 50, 100))
        if ok:
            S.expect[i] = f
        res.append(i)
    S.differ.append(tuple(res)); S.count("init.ratio", 2)
    # -- window: r = windowSize, a feature at exactly 10 px is no candidate
    x, y = S.anchor(); B = base_desc(); i = S.q(x, y, 0, B)
    S.feat(x + 10, y, 0, B); f = S.feat(dn(x + 10), y, 0, flip(B, 10, 50))
    assert F32(F32(x + 10) - x) == 10 and F32(dn(x + 10) - x) < 10
    S.expect[i] = f; S.count("init.window")
    # -- stealing (:633-634 `if (vMatchedDistance[i2] <= dist) continue;`, :649-654): equal distance is skipped, a smaller one steals and the owner loses
    x, y = S.anchor(); B = base_desc()
    f = S.feat(x + 1, y, 0, B)
    o1 = S.q(x, y, 0, flip(B, 20)); o2 = S.q(x, y, 0, flip(B, 20, 100))
    S.expect[o1] = f
    x, y = S.anchor(); B = base_desc()
    f = S.feat(x + 1, y, 0, B)
    o3 = S.q(x, y, 0, flip(B, 20)); o4 = S.q(x, y, 0, flip(B, 10, 100))
    S.expect[o4] = f
    S.differ += [(o1, o2), (o4, o3)]; S.count("init.stealing", 2)
    return S.problem()


def init_histogram(name):
    S = InitScene("init_hist_" + name, nnratio=0.9)
    _check_histogram(HISTOGRAMS[name])

    def pair(rot):
        x, y = S.anchor(); B = base_desc()
        i = S.q(x, y, 0, B, angle=F32(rot)); f = S.feat(x + 1, y, 0, flip(B, 10))
        return f, i           # expect[i] = f
    rows = _histogram(S, HISTOGRAMS[name], pair)
    kept = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and b[2]]; gone = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and not b[2]]
    S.differ += [(kept[0], g) for g in gone]
    S.count("init.rotation_histogram")
    return S.problem()


def init_problems():
    return [init_main(0.8), init_main(0.9)] + [init_histogram(n) for n in HISTOGRAMS]


# =========================================================================================================================================
# ORBmatcher::SearchForTriangulation (ORBmatcher.cc:821-1042), pinhole
# =========================================================================================================================================
class TriScene:
    def __init__(self, name, pyr="p12", onlyStereo=False, coarse=False, ori=True, ep=(-1000.0, -1000.0)):
        self.name, self.pyr, self.onlyStereo, self.coarse, self.ori = name, pyr, onlyStereo, coarse, ori
        self.ep = np.array(ep, F32)
        self.k1, self.k2, self.expect, self.differ, self.classes = [], [], {}, [], {}
        self._node = 0

    def node(self):
        self._node += 1
        return self._node

    def f1(self, x, y, desc, node, octave=0, angle=0.0, ur=-1.0, has=0):
        self.k1.append((F32(x), F32(y), int(octave), F32(angle), desc, int(node), F32(ur), int(has)))
        return len(self.k1) - 1

    def f2(self, x, y, desc, node, octave=0, angle=0.0, ur=-1.0, has=0):
        self.k2.append((F32(x), F32(y), int(octave), F32(angle), desc, int(node), F32(ur), int(has)))
        return len(self.k2) - 1

    def count(self, cls, n=1):
        self.classes[cls] = self.classes.get(cls, 0) + n

    def problem(self):
        def arr(rows):
            return dict(k=keypoints([r[:4] for r in rows]), d=np.stack([r[4] for r in rows]).astype(np.uint8), node=np.array([r[5] for r in rows], np.int32),
                        ur=np.array([r[6] for r in rows], F32), has=np.array([r[7] for r in rows], np.uint8))
        assert len(self.k1) <= 128 and len(self.k2) <= 128
        e = np.full(len(self.k1), -1, np.int32)
        for i, f in self.expect.items():
            e[i] = f
        return dict(entry="tri", name=self.name, pyr=self.pyr, onlyStereo=self.onlyStereo, coarse=self.coarse, ori=self.ori, ep=self.ep, F1=arr(self.k1),
                    F2=arr(self.k2), R12=np.eye(3, dtype=F32), t12=np.array([1.0, 0.0, 0.0], F32), expect=e, differ=list(self.differ),
                    classes=dict(self.classes))


def epipolar_dsqr(kp1, kp2):
    """Pinhole::epipolarConstrain's dsqr (Pinhole.cpp:111-139) in float32 for R12 = I, t12 = (1, 0, 0): F12 through orc_fundamental_f12's own products."""
    K = np.array([FX, FY, CX, CY], F32)
    k1it = np.array([1 / K[0], 0, 0, 0, 1 / K[1], 0, -K[2] / K[0], -K[3] / K[1], 1], F32)
    k2i = np.array([1 / K[0], 0, -K[2] / K[0], 0, 1 / K[1], -K[3] / K[1], 0, 0, 1], F32)
    tx = np.array([0, -0.0, 0, 0.0, 0, -1, -0.0, 1, 0], F32)

    def mul(A, B):
        return np.array([F32(F32(F32(A[i * 3] * B[j]) + F32(A[i * 3 + 1] * B[3 + j])) + F32(A[i * 3 + 2] * B[6 + j])) for i in range(3) for j in range(3)], F32)
    F12 = mul(mul(mul(k1it, tx), np.eye(3, dtype=F32).reshape(9)), k2i)
    x1, y1 = F32(kp1[0]), F32(kp1[1]); x2, y2 = F32(kp2[0]), F32(kp2[1])
    a = F32(F32(F32(x1 * F12[0]) + F32(y1 * F12[3])) + F12[6]); b = F32(F32(F32(x1 * F12[1]) + F32(y1 * F12[4])) + F12[7])
    c = F32(F32(F32(x1 * F12[2]) + F32(y1 * F12[5])) + F12[8])
    num = F32(F32(F32(a * x2) + F32(b * y2)) + c); den = F32(F32(a * a) + F32(b * b))
    return F32(F32(num * num) / den)


def tri_main():
    S = TriScene("tri_main", "p12")
    sg = sigma2("p12")
    # -- acceptance: bestDist starts at TH_LOW and `if (dist > TH_LOW || dist > bestDist) continue;` (:915-916): 50 is taken, 51 is not
    res = []
    for d in (TH_LOW, TH_LOW + 1):
        B = base_desc(); n = S.node(); y = F32(30 + 10 * len(S.k1))
        i = S.f1(100.0, y, B, n); f = S.f2(140.0, y, flip(B, d), n)
        if d == TH_LOW:
            S.expect[i] = f
        res.append(i)
    S.differ.append(tuple(res)); S.count("tri.acceptance", 2)
    # equal distances: `dist > bestDist` lets an equal candidate REPLACE the best: the last one of the node's list wins
    B = base_desc(); n = S.node(); y = F32(30 + 10 * len(S.k1))
    i = S.f1(100.0, y, B, n); S.f2(140.0, y, flip(B, 20), n); f = S.f2(150.0, y, flip(B, 20, 100), n)
    S.expect[i] = f; S.count("tri.tie_last_wins")
    # -- the epipolar line (Pinhole.cpp:136 `return dsqr < 3.84 * unc;`, in double): y2 either side of the bound at octave 0 (unc = 1) and 3
    for octave in (0, 3):
        bound = 3.84 * float(sg[octave])
        y1 = F32(200.0)
        y2 = F32(y1 + F32(np.sqrt(bound)))
        while float(epipolar_dsqr((100.0, y1), (160.0, y2))) < bound:
            y2 = up(y2)
        while float(epipolar_dsqr((100.0, y1), (160.0, y2))) >= bound:
            y2 = dn(y2)
        y2_out = up(y2)
        assert float(epipolar_dsqr((100.0, y1), (160.0, y2))) < bound <= float(epipolar_dsqr((100.0, y1), (160.0, y2_out)))
        res = []
        for yy, ok in ((y2, True), (y2_out, False)):
            B = base_desc(); n = S.node()
            i = S.f1(100.0, y1, B, n); f = S.f2(160.0, yy, flip(B, 10), n, octave=octave)
            if ok:
                S.expect[i] = f
            res.append(i)
        S.differ.append(tuple(res)); S.count("tri.epipolar_line", 2)
    # -- has a map point (:881-882, :905-906): neither side is matched
    B = base_desc(); n = S.node(); S.f1(100.0, 300.0, B, n, has=1); S.f2(140.0, 300.0, B, n)
    B = base_desc(); n = S.node(); S.f1(100.0, 310.0, B, n); S.f2(140.0, 310.0, B, n, has=1)
    S.count("tri.has_map_point", 2)
    return S.problem()


def tri_epipole():
    """:925-933: for two monocular features `if (distex * distex + distey * distey < 100 * scaleFactor) continue;`, with bCoarse so that the epipolar
    line plays no part.  ep = (200, 100); kp2 = ep + (6, 8): 36 + 64 = 100 == 100 * 1.0f is kept; octave 2 of (2.0, 3): 100 * 4 = 400 = 12^2 + 16^2."""
    out = []
    for pyr, octave, dx, dy in (("p12", 0, 6.0, 8.0), ("p20", 2, 12.0, 16.0)):
        S = TriScene("tri_epipole_" + pyr, pyr, coarse=True, ep=(200.0, 100.0))
        sf = scale_factors(pyr)
        lim = F32(F32(100) * sf[octave])
        d2 = lambda x, y: F32(F32(F32(F32(200.0) - F32(x)) * F32(F32(200.0) - F32(x))) + F32(F32(F32(100.0) - F32(y)) * F32(F32(100.0) - F32(y))))
        x_eq, y_eq = F32(200 + dx), F32(100 + dy)
        y_in = dn(y_eq)
        while not d2(x_eq, y_in) < lim:
            y_in = dn(y_in)
        y_out = up(y_eq)
        assert d2(x_eq, y_eq) == lim and d2(x_eq, y_in) < lim and d2(x_eq, y_out) >= lim
        res = {}
        for name, yy in (("eq", y_eq), ("in", y_in), ("out", y_out)):
            B = base_desc(); n = S.node()
            i = S.f1(50.0, F32(20 + 10 * n), B, n); f = S.f2(x_eq, yy, flip(B, 10), n, octave=octave)
            if name != "in":
                S.expect[i] = f
            res[name] = i
        # a stereo feature on either side is exempt from the epipole test (bStereo1 || bStereo2)
        B = base_desc(); n = S.node()
        i = S.f1(50.0, F32(20 + 10 * n), B, n, ur=40.0); f = S.f2(x_eq, y_in, flip(B, 10), n, octave=octave)
        S.expect[i] = f
        S.differ += [(res["eq"], res["in"]), (res["out"], res["in"]), (i, res["in"])]
        S.count("tri.epipole_distance", 4)
        out.append(S.problem())
    return out


def tri_only_stereo():
    out = []
    for only in (False, True):
        S = TriScene("tri_only_stereo_%d" % only, "p12", onlyStereo=only, coarse=True)
        res = []
        for ur1, ur2 in ((-1.0, -1.0), (40.0, -1.0), (-1.0, 40.0), (40.0, 40.0), (0.0, 0.0)):      # uRight == 0 counts as stereo (`>= 0`, :884)
            B = base_desc(); n = S.node()
            i = S.f1(50.0, F32(20 + 10 * n), B, n, ur=ur1); f = S.f2(300.0, F32(20 + 10 * n), flip(B, 10), n, ur=ur2)
            if not only or (ur1 >= 0 and ur2 >= 0):
                S.expect[i] = f
            res.append(i)
        if only:
            S.differ += [(res[3], res[0]), (res[3], res[1]), (res[3], res[2]), (res[4], res[0])]
        S.count("tri.only_stereo", 5)
        out.append(S.problem())
    return out


def tri_histogram(name):
    S = TriScene("tri_hist_" + name, "p12", coarse=True)
    _check_histogram(HISTOGRAMS[name])

    def pair(rot):
        B = base_desc(); n = S.node()
        i = S.f1(50.0, F32(20 + 5 * n), B, n, angle=F32(rot)); f = S.f2(300.0, F32(20 + 5 * n), flip(B, 10), n)
        return f, i
    rows = _histogram(S, HISTOGRAMS[name], pair)
    kept = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and b[2]]; gone = [r[0] for r, b in zip(rows, HISTOGRAMS[name]) if r and not b[2]]
    S.differ += [(kept[0], g) for g in gone]
    S.count("tri.rotation_histogram")
    return S.problem()


def tri_problems():
    return [tri_main()] + tri_epipole() + tri_only_stereo() + [tri_histogram(n) for n in HISTOGRAMS]


# =========================================================================================================================================
_ALL = {}


def problems(entry):
    """Every problem of an entry, built once."""
    if entry not in _ALL:
        _ALL[entry] = {
            "frustum": lambda: [frustum_main(), frustum_depth()] + [frustum_predict_scale(p) for p in PYRAMIDS],
            "mps": mps_problems, "last": last_problems, "kf": kf_problems, "fuse": kfproj_problems, "sim3": sim3_problems,
            "sim3dir": lambda: [sim3dir_problem()], "init": init_problems, "tri": tri_problems,
        }[entry]()
    return _ALL[entry]


ENTRIES = ("frustum", "mps", "last", "kf", "fuse", "sim3", "sim3dir", "init", "tri")


def class_counts():
    tot = {}
    for e in ENTRIES:
        for p in problems(e):
            for c, n in p["classes"].items():
                tot[c] = tot.get(c, 0) + n
    return tot


# =========================================================================================================================================
# the oracle on one problem: what both test files compare against
# =========================================================================================================================================
def oracle(p):
    """-> dict(table=the entry's main output (what `expect` describes), n=its match count or None, plus the entry's other outputs)."""
    P = params(p["pyr"])
    e = p["entry"]
    if e == "frustum":
        F = O.make_frame(P, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), None)
        with np.errstate(all="ignore"):
            o = O.is_in_frustum(F, p["R"].reshape(3, 3), p["t"], p["Ow"], p["Pw"], p["normal"], p["maxD"], p["minD"], p["cosLimit"])
        return dict(table=o["inView"], n=None, trk=o)
    if e == "mps":
        F = O.make_frame(P, p["k"], p["d"], p["ur"])
        q = p["q"]
        r, m = O.search_by_projection_mps(F, p["flag"], q, q["isBad"], q["mpDesc"], q["hasObs"], p["th"], p["bFar"], p["thFar"], p["nnratio"],
                                          match_init=p["init"])
        return dict(table=m, n=r)
    if e == "last":
        F = O.make_frame(P, p["k"], p["d"], p["ur"])
        r, m = O.search_by_projection_last(F, p["flag"], p["Tcw"], p["lastK"], p["lastValid"], p["lastXw"], p["lastDesc"], p["lastObs"], p["th"],
                                           p["fwd"], p["bwd"], p["ori"], match_init=p["init"])
        return dict(table=m, n=r)
    if e == "kf":
        F = O.make_frame(P, p["k"], p["d"], None)
        r, m = O.search_by_projection_kf(F, p["flag"], p["Tcw"], p["Ow"], p["lastK"], p["lastValid"], p["lastXw"], p["maxD"], p["minD"], p["lastDesc"],
                                         p["th"], p["orb"], p["ori"], match_init=p["init"])
        return dict(table=m, n=r)
    if e in ("fuse", "fuse_sim3"):
        F = O.make_frame(P, p["k"], p["d"], p["ur"])
        invS = (F32(1.0) / sigma2(p["pyr"])).astype(F32)
        bi, bd = O.fuse_search(F, invS, p["Tcw"], p["Ow"], p["valid"], p["Pw"], p["normal"], p["maxD"], p["minD"], p["mpDesc"], p["th"], p["sim3Form"])
        return dict(table=bi, n=None, dist=bd)
    if e == "sim3":
        F = O.make_frame(P, p["k"], p["d"], None)
        r, m = O.search_by_projection_sim3(F, p["Tcw"], p["Ow"], p["valid"], p["Pw"], p["normal"], p["maxD"], p["minD"], p["mpDesc"], p["flag"],
                                           int(p["th"]), p["ratio"], p["manual"])
        return dict(table=m, n=r)
    if e == "sim3dir":
        FA = O.make_frame(P, p["A"]["k"], p["A"]["d"], None); FB = O.make_frame(P, p["B"]["k"], p["B"]["d"], None)
        a, b = p["ptsA"], p["ptsB"]
        v1 = O.search_by_sim3_dir(FB, IDENTITY7, p["S"], a["valid"], a["Pw"], a["maxD"], a["minD"], a["mpDesc"], p["th"])
        v2 = O.search_by_sim3_dir(FA, IDENTITY7, p["S"], b["valid"], b["Pw"], b["maxD"], b["minD"], b["mpDesc"], p["th"])
        m12 = np.array([i2 if (i2 >= 0 and v2[i2] == i1) else -1 for i1, i2 in enumerate(v1)], np.int32)      # :1501-1516
        return dict(table=m12, n=int((m12 >= 0).sum()), v1=v1, v2=v2)
    if e == "init":
        F2 = O.make_frame(P, p["k2"], p["d2"], None)
        r, m, pv = O.search_for_initialization(p["k1"], p["d1"], F2, p["prev"], p["win"], p["nnratio"], p["ori"])
        return dict(table=m, n=r, prev=pv)
    if e == "tri":
        a, b = p["F1"], p["F2"]
        r, m = O.search_for_triangulation(a["k"], a["d"], a["node"], a["has"], a["ur"], b["k"], b["d"], b["node"], b["has"], b["ur"],
                                          list(P.levelSigma2)[:P.nlevels], list(P.scaleFactors)[:P.nlevels], [P.fx, P.fy, P.cx, P.cy], p["R12"],
                                          p["t12"], p["ep"], p["onlyStereo"], p["coarse"], p["ori"])
        return dict(table=m, n=r)
    raise KeyError(e)


def assigned(p, table):
    """Per output row: does it hold an assignment made by THIS call (not what the in/out table held on entry, not -1)?"""
    init = p.get("init")
    t = np.asarray(table)
    return (t >= 0) & (t != init) if init is not None and len(init) == len(t) else t >= 0
