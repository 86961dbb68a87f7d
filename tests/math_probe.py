"""Helpers of the device-math tests: the ctypes face of tests/native/libmath_probe.so (tests/native/math_probe_*.hip — the scalar, 3 x 3 and
wave-level device functions behind thin entry points), the input sets with the branch each input takes, and the references:
  * mpmath at 60 digits for everything real-valued.  A reference with a branch (exp_so3, se3_exp, sim3_exp, log_so3, the right Jacobians,
    R_to_q) evaluates the reference project's FORMULA, threshold branch included, at high precision — not the true exponential: at
    theta = 9.9e-6 the two differ and the kernel must follow the formula.  The same Python text runs on plain floats as the "FP64
    transcription" whose error against mpmath sets each bound (BOUNDS, measured by test_device_math_cpu.py);
  * numpy eigh / svd for the eigen and polar references;
  * a pure-Python model of the DPP scan of csrc/wave.h for the order of sum_f64 / row_sum_f64."""
import ctypes as C
import functools
import math
import os

import numpy as np

U = 2.0 ** -53                      # unit roundoff of FP64
EPS = 2.0 ** -52                    # one ulp of 1.0
_lib = None

# name -> (input dtype, values per input record, output dtype, values per output record, has a host entry)
MAPS = {
    "atanf": ("f4", 1, "f4", 1, True), "acosf": ("f4", 1, "f4", 1, True), "tanf": ("f4", 1, "f4", 1, True),
    "sinf": ("f4", 1, "f4", 1, True), "cosf": ("f4", 1, "f4", 1, True), "atan2f": ("f4", 2, "f4", 1, True),
    "sin64": ("f8", 1, "f8", 1, True), "cos64": ("f8", 1, "f8", 1, True), "sincos64": ("f8", 1, "f8", 2, True),
    "exp64": ("f8", 1, "f8", 1, True),
    "pinhole_project": ("f4", 11, "f4", 2, True), "pinhole_unproject": ("f4", 10, "f4", 3, True),
    "kb8_project": ("f4", 11, "f4", 2, True), "kb8_unproject": ("f4", 10, "f4", 3, True),
    "kb8_project_d": ("f8", 11, "f8", 2, True), "kb8_project_jac": ("f8", 11, "f8", 6, True),
    "q_rotate_d": ("f8", 7, "f8", 3, False), "q_rotate_f": ("f4", 7, "f4", 3, False), "q_to_R": ("f8", 4, "f8", 9, False),
    "R_to_q_se3": ("f8", 9, "f8", 4, False), "se3_normalize": ("f8", 7, "f8", 7, False), "se3_mul": ("f8", 14, "f8", 7, False),
    "se3_map": ("f8", 10, "f8", 3, False), "se3_from_float": ("f4", 7, "f8", 7, False), "se3_exp": ("f8", 6, "f8", 7, False),
    "cube_rn": ("f8", 1, "f8", 1, False), "huber": ("f8", 2, "f8", 2, False), "sin_small": ("f8", 1, "f8", 1, False),
    "R_to_q_sim3": ("f8", 9, "f8", 4, False), "sim3_exp": ("f8", 7, "f8", 8, False), "sim3_mul": ("f8", 16, "f8", 8, False),
    "sim3_inverse": ("f8", 8, "f8", 8, False), "sim3_map": ("f8", 11, "f8", 3, False), "sim3_roundtrip": ("f8", 11, "f8", 3, False),
    "exp_so3": ("f8", 3, "f8", 9, False), "log_so3": ("f8", 9, "f8", 3, False), "right_jacobian_so3": ("f8", 3, "f8", 9, False),
    "inv_right_jacobian_so3": ("f8", 3, "f8", 9, False), "normalize_rotation_f": ("f4", 9, "f4", 9, False),
}


def lib():
    """The probe library.  Loading it and calling host_* entries needs no GPU; torch first, so that it binds to the HIP runtime torch brought."""
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        from morb_slam_amd import build
        L = C.CDLL(os.environ.get("MORB_MATH_PROBE_LIB") or build.build_math_probe())   # (a scratch build with one thing broken points this at itself)
        vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_longlong, C.c_double
        for name, spec in MAPS.items():
            for pre in ("probe_",) + (("host_",) if spec[4] else ()):
                fn = getattr(L, pre + name)
                fn.restype, fn.argtypes = i32, [vp, vp, i64]
        L.probe_wave.restype, L.probe_wave.argtypes = i32, [i32, vp, vp, i32, i32, i32]
        L.probe_ransac_block.restype, L.probe_ransac_block.argtypes = i32, [i32, vp, i32, vp, vp]
        L.probe_invert_n.restype, L.probe_invert_n.argtypes = i32, [vp, i32, i64, vp, vp, vp]
        L.probe_clamp_eigenvalues.restype, L.probe_clamp_eigenvalues.argtypes = i32, [vp, i32, f64, i64, vp, vp]
        L.probe_row_jacobi.restype, L.probe_row_jacobi.argtypes = i32, [vp, i32, vp, vp]
        _lib = L
    return _lib


def _records(name, x):
    it, ni, ot, no, _ = MAPS[name]
    x = np.ascontiguousarray(np.asarray(x).view(np.dtype(it)) if np.asarray(x).dtype.kind == "u" else np.asarray(x, dtype=it)).reshape(-1, ni)
    return x, np.dtype(ot), no


def host(name, x):
    """The host build of the header over the records x: (n, values per output record)."""
    x, ot, no = _records(name, x)
    out = np.empty((x.shape[0], no), ot)
    st = getattr(lib(), "host_" + name)(x.ctypes.data, out.ctypes.data, x.shape[0])
    assert st == 0, (name, st)
    return out


def device(name, x):
    """The gfx950 build over the records x, one thread per record: (n, values per output record)."""
    import torch
    x, ot, no = _records(name, x)
    dx = torch.from_numpy(x).cuda()
    dout = torch.from_numpy(np.full((x.shape[0], no), 7, ot)).cuda()
    torch.cuda.synchronize()
    st = getattr(lib(), "probe_" + name)(dx.data_ptr(), dout.data_ptr(), x.shape[0])
    assert st == 0, (name, st)
    return dout.cpu().numpy()


def same_bits(a, b):
    """Mask of the entries with equal bits, NaN on both sides counting as equal."""
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))


def ulp_diff(a, b):
    """|a - b| in units in the last place, for finite doubles of one sign or straddling zero."""
    ia, ib = np.ascontiguousarray(a).view(np.int64).copy(), np.ascontiguousarray(b).view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    return np.abs(ia.astype(np.float64) - ib.astype(np.float64))


# ---- libm input sets -------------------------------------------------------------------------------------------------------------------
# every literal csrc/libm_f32.h compares its argument (or a word of it) against, as the float bit pattern, with the header line it is on
F32_LITERALS = {
    "atanf": [(0x4c000000, "38: |x| >= 2^25"), (0x7f800000, "39: NaN"), (0x3ee00000, "42: |x| < 0.4375"), (0x31000000, "43: |x| < 2^-29"),
              (0x3f980000, "47: |x| < 1.1875"), (0x3f300000, "48: |x| < 11/16"), (0x401c0000, "51: |x| < 2.4375")],
    "acosf": [(0x3f800000, "68, 69: |x| == 1, > 1"), (0x3f000000, "70: |x| < 0.5"), (0x32800000, "71: |x| <= 2^-26")],
    "tanf": [(0x3f490fda, "188: |x| <= pi/4"), (0x42f00000, "189: top > 0x42e, |x| >= 120"), (0x39000000, "150: |x| < 2^-13"),
             (0x3f2ca140, "157, 170: |x| >= 0.6744"), (0x3f800000, "151: (int)x == 0"),
             # reduce_fast at 192 - 193: n changes at the odd multiples of pi/4; 161: pio4 - x below 2^-13
             (0x4016cbe4, "192: 3 pi/4"), (0x407b53d1, "192: 5 pi/4"), (0x40afeddf, "192: 7 pi/4"), (0x3fc90fdb, "195: pi/2"), (0x40490fdb, "192: pi")],
    "sinf": [(0x3f400000, "219, 222: top < top(pi/4), the 2^20-granular word"), (0x39800000, "220, 224: top < top(2^-12)"),
             (0x3f490fdb, "230: n = 0 | 1 at pi/4"), (0x4016cbe4, "230: 3 pi/4"), (0x407b53d1, "230: 5 pi/4"), (0x40afeddf, "230: 7 pi/4"),
             (0x3fc90fdb, "230: pi/2"), (0x40490fdb, "230: pi"), (0x42f00000, "198: valid for |y| < 120")],
}
F32_LITERALS["cosf"] = F32_LITERALS["sinf"]
F32_DOMAIN = {"sinf": 120.0, "cosf": 120.0}   # libm_f32.h:198 "valid for |y| < 120": beyond, (int32_t)r overflows, which C++ leaves undefined


def _neigh32(bits, k=2048):
    b = np.arange(bits - k, bits + k + 1, dtype=np.int64)
    b = b[(b >= 0) & (b <= 0x7fffffff)].astype(np.uint32)
    return np.concatenate([b, b | np.uint32(0x80000000)])


@functools.lru_cache(maxsize=None)
def f32_inputs(name):
    """uint32 bit patterns: every 257th of all 2^32, +-2048 neighbours of every literal of the function (both signs), every 1024th denormal,
    +-0, +-inf, NaNs.  sinf / cosf: cut to the header's documented domain."""
    parts = [np.arange(0, 1 << 32, 257, dtype=np.uint64).astype(np.uint32)]
    parts += [_neigh32(b) for b, _ in F32_LITERALS[name]]
    den = np.arange(0, 0x00800000, 1024, dtype=np.uint32)
    parts += [den, den | np.uint32(0x80000000)]
    parts.append(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xff800001, 0x7fa00000], np.uint32))
    u = np.concatenate(parts)
    if name in F32_DOMAIN:
        u = u[np.abs(u.view(np.float32)) < F32_DOMAIN[name]]      # (drops NaN and inf too: the conversion is undefined for them as well)
    return u


@functools.lru_cache(maxsize=None)
def atan2f_inputs():
    """(y, x) uint32 pairs: 4 M pairs of random bit patterns and the full cross product of the special values."""
    rng = np.random.default_rng(0xA7A2)
    rnd = rng.integers(0, 1 << 32, (1 << 22, 2), dtype=np.uint64).astype(np.uint32)
    pos = [0x00000000, 0x00000001, 0x00000400, 0x007fffff, 0x00800000,            # zero, denormals, the smallest normal
           0x3f800000, 0x3f7fffff, 0x3f800001,                                     # 1 (e_atan2f.c: x == 1) and its neighbours
           0x7f7fffff, 0x7e800000, 0x5d800000, 0x5e000000, 0x5e800000,             # huge; 2^60, 2^61, 2^62: the k > 60 / k < -60 ratios against 1
           0x21000000, 0x20800000, 0x21800000,                                     # 2^-61, 2^-62, 2^-60
           0x7f800000,                                                             # inf
           0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000, 0x31000000,   # atanf's branch points as ratios against 1
           0x3edfffff, 0x3f2fffff, 0x3f97ffff, 0x401bffff, 0x4bffffff, 0x30ffffff,
           0x40000000, 0x3f000000, 0x40490fdb]
    sp = np.array(pos + [p | 0x80000000 for p in pos], np.uint32)
    assert len(sp) == 64
    yy, xx = np.meshgrid(sp, sp, indexing="ij")
    return np.concatenate([rnd, np.stack([yy.ravel(), xx.ravel()], 1)])


F64_LIMIT = 105414350.0    # libm_f64.h:2, :215
# the arguments csrc/libm_f64.h branches at (high-word compares at :218-220, :227-230, :246-248; do_sin's TAYLOR_SIN at :181)
F64_SINCOS_LITERALS = [(2.0 ** -26, "218: k < 0x3e500000"), (2.0 ** -27, "228, 247: k < 0x3e400000"), (0.126, "181: TAYLOR_SIN"),
                       (float.fromhex("0x1.b6p-1"), "219, 229, 248: k < 0x3feb6000 (0.855469)"),
                       (float.fromhex("0x1.368fdp+1"), "220, 230, 246: k < 0x400368fd (2.426265)")] + \
                      [((2 * k + 1) * math.pi / 4, "202-205: reduce_sincos quadrant boundary") for k in range(1, 12)] + \
                      [(k * math.pi / 2, "202-205: reduce_sincos, remainder through zero") for k in range(2, 8)]


def _neigh64(x, k=2048, below_only=False):
    b = np.float64(x).view(np.int64) + np.arange(-k, (0 if below_only else k + 1), dtype=np.int64)
    v = b.view(np.float64)
    return np.concatenate([v, -v])


@functools.lru_cache(maxsize=None)
def f64_sincos_inputs():
    rng = np.random.default_rng(0x51C0)
    k = np.arange(-int(math.pi * 2 ** 20), int(math.pi * 2 ** 20) + 1, dtype=np.float64) * 2.0 ** -20          # float-valued angles
    e = rng.uniform(math.log(1e-300), math.log(F64_LIMIT), 1 << 22)
    lu = np.exp(e) * rng.choice([-1.0, 1.0], 1 << 22)
    lu = lu[np.abs(lu) < F64_LIMIT]
    parts = [k, lu] + [_neigh64(x) for x, _ in F64_SINCOS_LITERALS] + [_neigh64(F64_LIMIT, below_only=True), np.array([0.0, -0.0])]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def f64_exp_inputs():
    """exp_glibc: [-40, 40], the 2^-54 threshold (libm_f64.h:339) and the restated range |x| < 512 (:264) up to its limit."""
    rng = np.random.default_rng(0xE4B)
    parts = [rng.uniform(-40, 40, 1 << 22), _neigh64(2.0 ** -54), _neigh64(512.0, below_only=True), _neigh64(math.log(2) / 256),
             np.exp(rng.uniform(math.log(1e-300), math.log(512.0), 1 << 20)) * rng.choice([-1.0, 1.0], 1 << 20), np.array([0.0, -0.0])]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def sin_small_inputs():
    """|x| < 0.126 (optimizer_device.h: sin_glibc_small's restated range), with the neighbours of 2^-26 and those of 0.126 below it."""
    rng = np.random.default_rng(0x5A11)
    lu = np.exp(rng.uniform(math.log(1e-12), math.log(0.126), 1 << 22)) * rng.choice([-1.0, 1.0], 1 << 22)
    x = np.concatenate([lu, rng.uniform(-0.126, 0.126, 1 << 20), _neigh64(2.0 ** -26), _neigh64(0.126), np.array([0.0, -0.0])])
    return x


# ---- camera input sets -----------------------------------------------------------------------------------------------------------------
PINHOLE = np.array([458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0], np.float32)
KB8 = np.array([190.978, 190.973, 254.932, 256.897, 0.00348, 0.000715, -0.00205, 0.000203], np.float32)
KB8_B = np.array([285.7, 286.1, 420.3, 403.9, -0.0073, 0.0435, -0.0412, 0.0077], np.float32)
CAM_N = 1 << 20


@functools.lru_cache(maxsize=None)
def camera_points(kb8):
    """(n, 3) float64 points, depth 1e-3 .. 1e3 log-uniform.  kb8: incidence angles up to and beyond 90 degrees (z <= 0), points on the
    optical axis (r = 0, both signs of z), and the signed-zero / axis-aligned azimuths."""
    rng = np.random.default_rng(0xCA3 + kb8)
    d = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), CAM_N))
    if not kb8:
        xy = rng.uniform(-1.2, 1.2, (CAM_N, 2)) * d[:, None]
        return np.column_stack([xy, d])
    inc = rng.uniform(0, math.radians(135), CAM_N)
    inc[:1024] = math.radians(90) + rng.uniform(-1e-4, 1e-4, 1024)
    az = rng.uniform(-math.pi, math.pi, CAM_N)
    P = np.column_stack([d * np.sin(inc) * np.cos(az), d * np.sin(inc) * np.sin(az), d * np.cos(inc)])
    P[1024:1536, :2] = 0.0                                                     # r = 0 on the axis
    P[1536:1600, :2] = 0.0; P[1536:1600, 2] *= -1                              # ... and behind the camera
    P[1600:1700, 1] = 0.0; P[1700:1800, 0] = 0.0; P[1800:1850, 1] = -0.0
    return P


@functools.lru_cache(maxsize=None)
def camera_pixels():
    """(n, 2) float32 pixels: inside a 512 x 512 image, at its corners, and well outside them."""
    rng = np.random.default_rng(0xC1F)
    px = rng.uniform(-300, 900, (CAM_N, 2))
    corners = np.array([[0, 0], [511, 0], [0, 511], [511, 511], [-0.5, -0.5], [511.5, 511.5], [254.932, 256.897], [5000, -5000]])
    px[:len(corners)] = corners
    px[8:72] = KB8[2:4].astype(np.float64) + rng.uniform(-1e-5, 1e-5, (64, 2))      # theta_d around the 1e-8 test
    return px.astype(np.float32)


def cam_records(cam, tail, dtype):
    return np.column_stack([np.broadcast_to(cam.astype(dtype), (len(tail), 8)), tail.astype(dtype)])


# ---- SE3 / SO3 / Sim3: one text, two precisions --------------------------------------------------------------------------------------------
class F64:
    """plain Python floats: IEEE FP64, one rounding per operation, the host libm"""
    num = staticmethod(float)
    sqrt, sin, cos, acos, exp = (staticmethod(f) for f in (math.sqrt, math.sin, math.cos, math.acos, math.exp))

    @staticmethod
    def cube(x):
        return math.pow(x, 3)


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


class MP:
    """mpmath at 60 digits; inputs are the doubles the device reads, taken exactly"""
    @staticmethod
    def num(x):
        return _mp().mpf(float(x)) if not isinstance(x, _mp().mpf) else x

    sqrt = staticmethod(lambda x: _mp().sqrt(x))
    sin = staticmethod(lambda x: _mp().sin(x))
    cos = staticmethod(lambda x: _mp().cos(x))
    acos = staticmethod(lambda x: _mp().acos(x))
    exp = staticmethod(lambda x: _mp().exp(x))
    cube = staticmethod(lambda x: x * x * x)


def _hat(w, B):
    z = B.num(0)
    return [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]


def _mm(A, Bm):
    return [A[3 * i] * Bm[j] + A[3 * i + 1] * Bm[3 + j] + A[3 * i + 2] * Bm[6 + j] for i in range(3) for j in range(3)]


def _eye(B, k):
    return B.num(1 if k % 4 == 0 else 0)


def R_to_q(m, B):
    """Eigen's Quaternion(Matrix3) (Quaternion.h): (q = x y z w, branch 0 = trace > 0, 1 + i = largest diagonal i)."""
    t = m[0] + m[4] + m[8]
    q = [None] * 4
    if t > 0:
        t = B.sqrt(t + 1)
        q[3] = t / 2
        t = B.num(0.5) / t
        q[0], q[1], q[2] = (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
        return q, 0
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[i * 4]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = B.sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1)
    q[i] = t / 2
    t = B.num(0.5) / t
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return q, 1 + i


def q_normalized(q, B):
    """SE3Quat::normalizeRotation: w >= 0, unit norm"""
    if q[3] < 0:
        q = [-c for c in q]
    n = B.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def se3_exp(u, B, force=None):
    """SE3Quat::exp (g2o se3quat.h): (q, t, small-angle branch taken).  force: the branch to take (see lie_case)."""
    u = [B.num(c) for c in u]
    w = u[:3]
    theta = B.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = _hat(w, B)
    Om2 = _mm(Om, Om)
    small = theta < B.num(0.00001) if force is None else bool(force)
    if small:
        R = [_eye(B, k) + Om[k] + Om2[k] for k in range(9)]
        V = R
    else:
        s, c = B.sin(theta), B.cos(theta)
        a, b, cc = s / theta, (1 - c) / (theta * theta), (theta - s) / B.cube(theta)
        R = [_eye(B, k) + a * Om[k] + b * Om2[k] for k in range(9)]
        V = [_eye(B, k) + b * Om[k] + cc * Om2[k] for k in range(9)]
    q, _ = R_to_q(R, B)
    t = [V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5] for i in range(3)]
    return q_normalized(q, B) + t, small


def exp_so3(w, B, force=None):
    """ExpSO3 (G2oTypes.cc:783-796)"""
    w = [B.num(c) for c in w]
    d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    d = B.sqrt(d2)
    W = _hat(w, B)
    WW = _mm(W, W)
    small = d < B.num(1e-5) if force is None else bool(force)
    if small:
        return [_eye(B, k) + W[k] + B.num(0.5) * WW[k] for k in range(9)], small
    s, c = B.sin(d), B.cos(d)
    return [_eye(B, k) + W[k] * s / d + WW[k] * (1 - c) / d2 for k in range(9)], small


def log_so3(R, B, force=None):
    """LogSO3 (G2oTypes.cc:798-811): (w, branch: 0 general, 1 costheta outside [-1, 1], 2 |sin theta| < 1e-5)"""
    R = [B.num(c) for c in R]
    tr = R[0] + R[4] + R[8]
    w = [(R[7] - R[5]) / 2, (R[2] - R[6]) / 2, (R[3] - R[1]) / 2]
    ct = (tr - 1) * B.num(0.5)
    if (ct > 1 or ct < -1) if force is None else force == 1:
        return w, 1
    th = B.acos(ct)
    s = B.sin(th)
    if abs(s) < B.num(1e-5) if force is None else force == 2:
        return w, 2
    return [th * c / s for c in w], 0


def right_jacobian_so3(v, B, inverse=False, force=None):
    """RightJacobianSO3 / InverseRightJacobianSO3 (G2oTypes.cc:817-848)"""
    v = [B.num(c) for c in v]
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = B.sqrt(d2)
    W = _hat(v, B)
    small = d < B.num(1e-5) if force is None else bool(force)
    if small:
        return [_eye(B, k) for k in range(9)], small
    WW = _mm(W, W)
    if inverse:
        k2 = 1 / d2 - (1 + B.cos(d)) / (2 * d * B.sin(d))
        return [_eye(B, k) + W[k] / 2 + WW[k] * k2 for k in range(9)], small
    return [_eye(B, k) - W[k] * (1 - B.cos(d)) / d2 + WW[k] * (d - B.sin(d)) / (d2 * d) for k in range(9)], small


def sim3_exp(u, B, force=None):
    """Sim3(Vector7d) (g2o types/sim3.h): (q, t, s, branch = 2 * (|sigma| < eps) + smallRot)"""
    u = [B.num(c) for c in u]
    w, sigma = u[:3], u[6]
    s = B.exp(sigma)
    theta = B.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = _hat(w, B)
    Om2 = _mm(Om, Om)
    eps = B.num(0.00001)
    small = theta < eps if force is None else bool(force & 1)
    ssig = abs(sigma) < eps if force is None else bool(force & 2)
    one = B.num(1)
    if ssig:
        Cc = one
        if small:
            A, Bb = one / 2, one / 6
        else:
            sn, cs = B.sin(theta), B.cos(theta)
            th2 = theta * theta
            A, Bb = (1 - cs) / th2, (theta - sn) / (th2 * theta)
    else:
        Cc = (s - 1) / sigma
        if small:
            s2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / s2
            Bb = ((B.num(0.5) * s2 - sigma + 1) * s) / (s2 * sigma)
        else:
            sn, cs = B.sin(theta), B.cos(theta)
            a, b = s * sn, s * cs
            th2, s2 = theta * theta, sigma * sigma
            c = th2 + s2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            Bb = (Cc - ((b - 1) * sigma + a * theta) / c) * 1 / th2
    if small:
        R = [_eye(B, k) + Om[k] + Om2[k] for k in range(9)]
    else:
        sn, cs = B.sin(theta), B.cos(theta)
        f1, f2 = sn / theta, (1 - cs) / (theta * theta)
        R = [_eye(B, k) + f1 * Om[k] + f2 * Om2[k] for k in range(9)]
    q, _ = R_to_q(R, B)
    W = [A * Om[k] + Bb * Om2[k] + Cc * _eye(B, k) for k in range(9)]
    t = [W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5] for i in range(3)]
    return q + t + [s], 2 * int(ssig) + int(small)


def q_rotate(q, v, B):
    """the rotation of v by the unit quaternion q = x y z w, from the rotation matrix"""
    x, y, z, w = q
    R = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return [R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2] for i in range(3)], R


def q_mul(p, o):
    return [p[3] * o[0] + p[0] * o[3] + p[1] * o[2] - p[2] * o[1], p[3] * o[1] + p[1] * o[3] + p[2] * o[0] - p[0] * o[2],
            p[3] * o[2] + p[2] * o[3] + p[0] * o[1] - p[1] * o[0], p[3] * o[3] - p[0] * o[0] - p[1] * o[1] - p[2] * o[2]]


class F32:
    """numpy float32 scalars: IEEE FP32, one rounding per operation"""
    num = staticmethod(np.float32)
    sqrt = staticmethod(np.sqrt)


def q_rotate_eigen(q, v, B):
    """QuaternionBase::_transformVector: v + w (2 u x v) + u x (2 u x v)"""
    ux, uy, uz, w = q
    a, b, c = uy * v[2] - uz * v[1], uz * v[0] - ux * v[2], ux * v[1] - uy * v[0]
    a, b, c = a + a, b + b, c + c
    return [v[0] + w * a + (uy * c - uz * b), v[1] + w * b + (uz * a - ux * c), v[2] + w * c + (ux * b - uy * a)]


def q_to_R(q, B):
    """Quaternion::toRotationMatrix"""
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def se3_mul(a, b, B):
    """SE3Quat::operator*: (q_a q_b normalised, t_a + q_a t_b)"""
    rt = q_rotate_eigen(a[:4], b[4:7], B)
    return q_normalized(q_mul(a[:4], b[:4]), B) + [a[4 + i] + rt[i] for i in range(3)]


def huber(delta, e, B, force=None):
    """RobustKernelHuber::robustify: (rho, w, branch: 1 = beyond delta^2)"""
    dsqr = delta * delta
    if (e <= dsqr) if force is None else not force:
        return [e, B.num(1)], 0
    sq = B.sqrt(e)
    return [2 * sq * delta - dsqr, delta / sq], 1


# ---- input ladders --------------------------------------------------------------------------------------------------------------------------
# the issue's ladder, and 5e-5: the first theta at which the second-order branch and the closed form differ by more than the 4-ulp floor
# (theta^3 / 6 = 2e-14), so that a threshold moved upwards shows in the rotation itself
THETAS = (0.0, 1e-12, 9.999e-6, 1e-5, 1.0001e-5, 5e-5, 1e-3, 0.125, 0.127, 1.0, 3.0, math.pi - 1e-6)
SIGMAS = (0.0, 9.99e-6, -9.99e-6, 1e-5, -1e-5, 1.01e-5, -1.01e-5, 0.1, -0.1, 1.0, -1.0)
R_TO_Q_ANGLES = (0.0, 1e-8, 1e-5, 1.0, math.pi - 1e-3, math.pi - 1e-8, math.pi)


@functools.lru_cache(maxsize=None)
def axes(nrandom, seed=0):
    """unit axes: the three coordinate axes, the four diagonals (and a face diagonal per plane), then random ones"""
    rng = np.random.default_rng(0xA8E5 + seed)
    fixed = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]]
    a = np.array(fixed + list(rng.normal(size=(nrandom, 3))), np.float64)
    return a / np.linalg.norm(a, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def omega_ladder(nrandom=30):
    """(labels, (n, 3) rotation vectors): every theta of THETAS times every axis"""
    ax = axes(nrandom)
    lab, w = [], []
    for th in THETAS:
        for a in ax:
            lab.append(th)
            w.append(th * a)
    return np.array(lab), np.array(w)


@functools.lru_cache(maxsize=None)
def se3_exp_inputs():
    lab, w = omega_ladder()
    rng = np.random.default_rng(0x5E3)
    t = rng.uniform(-1, 1, (len(w), 3)) * 10.0 ** rng.uniform(-2, 2, (len(w), 1))       # translations up to 1e2
    return lab, np.column_stack([w, t])


@functools.lru_cache(maxsize=None)
def sim3_exp_inputs():
    """(theta labels, sigma labels, (n, 7) updates): THETAS x SIGMAS x 13 axes"""
    ax = axes(3, seed=1)
    rng = np.random.default_rng(0x513)
    lt, ls, u = [], [], []
    for th in THETAS:
        for sg in SIGMAS:
            for a in ax:
                lt.append(th); ls.append(sg)
                u.append(list(th * a) + list(rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-2, 2)) + [sg])
    return np.array(lt), np.array(ls), np.array(u)


@functools.lru_cache(maxsize=None)
def rotation_matrices():
    """(angle labels, (n, 9) doubles): Rodrigues' formula at 60 digits, rounded once, R_TO_Q_ANGLES x 150 axes"""
    mp = _mp()
    ax = axes(140, seed=2)
    lab, out = [], []
    for ang in R_TO_Q_ANGLES:
        s, c = mp.sin(mp.mpf(ang)), mp.cos(mp.mpf(ang))
        for a in ax:
            n = [mp.mpf(float(v)) for v in a]
            nn = mp.sqrt(n[0] ** 2 + n[1] ** 2 + n[2] ** 2)
            n = [v / nn for v in n]
            K = _hat(n, MP)
            KK = _mm(K, K)
            out.append([float(_eye(MP, k) + s * K[k] + (1 - c) * KK[k]) for k in range(9)])
            lab.append(ang)
    return np.array(lab), np.array(out)


@functools.lru_cache(maxsize=None)
def log_so3_inputs():
    """(class labels, (n, 9) matrices):
      'rt <theta>'   exp_so3 outputs (the FP64 transcription's) for theta from 1e-8 to pi - 1e-6;
      'out+' 'out-'  matrices whose trace puts costheta just outside [-1, 1];
      'sin0' 'sinpi' rotations with |sin theta| < 1e-5 at either end."""
    ax = axes(30, seed=3)
    lab, out = [], []
    for th in (1e-8, 1e-6, 2e-5, 1e-3, 0.5, 1.5, 3.0, math.pi - 1e-3, math.pi - 2e-5, math.pi - 1e-6):
        for a in ax:
            lab.append("rt %g" % th)
            out.append(exp_so3(list(th * a), F64)[0])
    rot = {th: [exp_so3(list(th * a), F64)[0] for a in ax] for th in (0.0, 3e-6, 9e-6, math.pi - 3e-6, math.pi - 9e-6, math.pi)}
    for th, name in ((3e-6, "sin0"), (9e-6, "sin0"), (math.pi - 3e-6, "sinpi"), (math.pi - 9e-6, "sinpi"), (math.pi, "sinpi")):
        for R in rot[th]:
            lab.append(name)
            out.append(R)
    for k, R in enumerate(rot[0.0] + rot[3e-6]):                    # trace above 3: the diagonal pushed up by 1 .. 40 ulp
        R = list(R)
        R[0] = 1.0 + (1 + k) * EPS
        lab.append("out+")
        out.append(R)
    for k, R in enumerate(rot[math.pi] + rot[math.pi - 3e-6]):      # trace below -1: the diagonal scaled by 1 + 2^-40 .. 2^-30
        s = 1.0 + 2.0 ** -(30 + k % 11)
        lab.append("out-")
        out.append([c * s for c in R])
    return np.array(lab), np.array(out, np.float64)


def nerr(out, ref, groups):
    """per record: the largest |out - ref| of each group of output entries over the largest |ref| of the group (1 where that is 0), the
    worst group.  out: (n, k) doubles, ref: (n, k) of mpmath numbers (object array)."""
    n = len(out)
    worst = np.zeros(n)
    for i in range(n):
        for g in groups:
            sc = max(abs(ref[i][k]) for k in g)
            e = max(abs(_mp().mpf(float(out[i][k])) - ref[i][k]) for k in g)
            worst[i] = max(worst[i], float(e / sc) if sc != 0 else float(e))
    return worst


def quat_sign_aligned(q, ref):
    """q with the sign that matches ref (q and -q are one rotation)"""
    q = np.array(q, np.float64)
    for i in range(len(q)):
        if sum(float(q[i][k]) * float(ref[i][k]) for k in range(4)) < 0:
            q[i, :4] = -q[i, :4]
    return q


G_Q = (range(0, 4),)
G_SE3 = (range(0, 4), range(4, 7))
G_SIM3 = (range(0, 4), range(4, 7), range(7, 8))
G_M33 = (range(0, 9),)
G_V3 = (range(0, 3),)


ALGEBRA = ("q_rotate_d", "q_rotate_f", "q_to_R", "se3_normalize", "se3_mul", "se3_map", "se3_from_float", "cube_rn", "huber")
HUBER_DELTAS = (math.sqrt(5.991), math.sqrt(7.815), 1.0, 3.0)      # the chi2 thresholds of the optimisers, and two exact squares


def algebra_case(name):
    """(labels, inputs, f(row, B, force) -> (values, branch), groups) of the branch-free primitives (huber: one branch, on exact data)"""
    rng = np.random.default_rng(0xA16 + sum(map(ord, name)))
    n = 512
    lab = np.array(["all"] * n)

    def quats(k, dtype=np.float64):
        q = rng.normal(size=(k, 4))
        q[: k // 8, 3] = -np.abs(q[: k // 8, 3]) * 1e-3                        # w < 0 and small: the sign flip of the normalisation
        return (q / np.linalg.norm(q, axis=1)[:, None]).astype(dtype).astype(np.float64)

    def vecs(k, dtype=np.float64):
        return (rng.uniform(-1, 1, (k, 3)) * 10.0 ** rng.uniform(-2, 2, (k, 1))).astype(dtype).astype(np.float64)
    nums = lambda row, B: [B.num(c) for c in row]
    if name in ("q_rotate_d", "q_rotate_f"):
        dt = np.float32 if name.endswith("f") else np.float64
        x = np.column_stack([quats(n, dt), vecs(n, dt)])
        f = lambda row, B, force=None: (q_rotate_eigen(nums(row, B)[:4], nums(row, B)[4:], B), 0)
        return lab, x, f, G_V3
    if name == "q_to_R":
        return lab, quats(n), (lambda row, B, force=None: (q_to_R(nums(row, B), B), 0)), G_M33
    if name == "se3_normalize":
        x = np.column_stack([quats(n) * rng.uniform(0.5, 2, (n, 1)), vecs(n)])
        return lab, x, (lambda row, B, force=None: (q_normalized(nums(row, B)[:4], B) + nums(row, B)[4:], 0)), G_SE3
    if name == "se3_from_float":
        x = np.column_stack([quats(n, np.float32), vecs(n, np.float32)])
        return lab, x, (lambda row, B, force=None: (q_normalized(nums(row, B)[:4], B) + nums(row, B)[4:], 0)), G_SE3
    if name == "se3_mul":
        x = np.column_stack([quats(n), vecs(n), quats(n), vecs(n)])
        return lab, x, (lambda row, B, force=None: (se3_mul(nums(row, B)[:7], nums(row, B)[7:], B), 0)), G_SE3
    if name == "se3_map":
        x = np.column_stack([quats(n), vecs(n), vecs(n)])

        def f(row, B, force=None):
            r = nums(row, B)
            o = q_rotate_eigen(r[:4], r[7:], B)
            return [o[i] + r[4 + i] for i in range(3)], 0
        return lab, x, f, G_V3
    if name == "cube_rn":
        x = np.concatenate([np.array(THETAS[1:]), rng.uniform(0, math.pi, n - len(THETAS) + 1)])[:, None]
        return lab, x, (lambda row, B, force=None: ([B.cube(B.num(row[0]))], 0)), (range(0, 1),)
    if name == "huber":
        rows = []
        for d in HUBER_DELTAS:
            d2 = np.float64(d) * np.float64(d)                                 # delta^2 as the kernel rounds it
            rows += [[d, d2], [d, np.nextafter(d2, 0)], [d, np.nextafter(d2, np.inf)], [d, 0.0]]
            rows += [[d, e] for e in d2 * 10.0 ** rng.uniform(-6, 6, n // len(HUBER_DELTAS) - 4)]
        x = np.array(rows)
        lab = np.array(["all"] * len(x))
        return lab, x, (lambda row, B, force=None: huber(B.num(row[0]), B.num(row[1]), B, force)), (range(0, 1), range(1, 2))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def lie_case(name):
    """(labels, inputs (n, ni), reference rows (mpmath), transcription rows (float), branch per input, groups) of one primitive."""
    if name == "se3_exp":
        lab, x = se3_exp_inputs()
        f, groups = se3_exp, G_SE3
    elif name == "exp_so3":
        lab, x = omega_ladder()
        f, groups = exp_so3, G_M33
    elif name == "right_jacobian_so3":
        lab, x = omega_ladder()
        f, groups = right_jacobian_so3, G_M33
    elif name == "inv_right_jacobian_so3":
        lab, x = omega_ladder()
        f, groups = (lambda v, B, force=None: right_jacobian_so3(v, B, inverse=True, force=force)), G_M33
    elif name == "log_so3":
        lab, x = log_so3_inputs()
        f, groups = log_so3, G_V3
    elif name == "sim3_exp":
        lt, ls, x = sim3_exp_inputs()
        lab = np.array(["%g|%g" % (a, abs(b)) for a, b in zip(lt, ls)])
        f, groups = sim3_exp, G_SIM3
    elif name == "R_to_q":
        lab, x = rotation_matrices()
        f, groups = (lambda m, B, force=None: R_to_q([B.num(c) for c in m], B)), G_Q
    elif name in ALGEBRA:
        lab, x, f, groups = algebra_case(name)
    else:
        raise KeyError(name)
    ref, tr, br = [], [], []
    for row in x:
        t, b = f(list(row), F32 if name == "q_rotate_f" else F64)
        r, b2 = f(list(row), MP, force=b)      # the reference takes the branch the FP64 arithmetic takes: an input whose
        assert b2 == b                          # rounded theta lands on the threshold has no other well-defined answer
        ref.append(r); tr.append(t); br.append(int(b))
    return lab, x, ref, np.array(tr, np.float64), np.array(br), groups


def class_errors(name, out):
    """{label: largest nerr of `out` over the inputs of that label}"""
    lab, x, ref, tr, br, groups = lie_case(name)
    if name in ("R_to_q",):
        out = quat_sign_aligned(out, ref)
    e = nerr(out, ref, groups)
    return {str(l): float(e[lab == l].max()) for l in dict.fromkeys(lab.tolist())}


FLOOR = 4 * EPS     # 4 ulp of the largest output entry (nerr is relative to it)
DEVICE_FACTOR = 8   # the device library's sin / cos / acos / sqrt within the OpenCL full-profile bounds, against the host's 1 ulp

# The largest nerr of the FP64 transcription (the functions above on Python floats, host libm) against mpmath, per primitive and input
# class, rounded up to two digits; test_device_math_cpu.py measures them again and holds each to [value / 2, value].  The device is held to
# max(DEVICE_FACTOR * value, FLOOR).  A class dominated by cancellation in the formula itself (1 - cos(theta) at theta = 1e-5, acos next to
# +-1) has a large value: the formula is that ill-conditioned there, in any FP64 arithmetic.
BOUNDS = {
    "se3_exp": {"0.0": 0, "1e-12": 1.6e-16, "9.999e-06": 2.4e-16, "1e-05": 5.3e-13, "1.0001e-05": 5.4e-13, "5e-05": 1.9e-13, "0.001": 1.1e-14,
        "0.125": 5e-16, "0.127": 2.2e-16, "1.0": 1.8e-16, "3.0": 3.4e-16, "3.141591653589793": 3.6e-16},
    "exp_so3": {"0.0": 0, "1e-12": 5e-25, "9.999e-06": 5.6e-17, "1e-05": 5.7e-17, "1.0001e-05": 5.9e-17, "5e-05": 6.2e-17, "0.001": 6.3e-17,
        "0.125": 1.1e-16, "0.127": 6.3e-17, "1.0": 2.9e-16, "3.0": 5.2e-16, "3.141591653589793": 5.4e-16},
    "right_jacobian_so3": {"0.0": 0, "1e-12": 0, "9.999e-06": 0, "1e-05": 4.2e-13, "1.0001e-05": 4.4e-13, "5e-05": 1.5e-13, "0.001": 7.9e-15,
        "0.125": 3.9e-16, "0.127": 1.2e-16, "1.0": 2.1e-16, "3.0": 2.6e-16, "3.141591653589793": 3.3e-16},
    "inv_right_jacobian_so3": {"0.0": 0, "1e-12": 0, "9.999e-06": 0, "1e-05": 3.5e-16, "1.0001e-05": 3.4e-16, "5e-05": 3.9e-16, "0.001": 2.2e-16,
        "0.125": 3.2e-16, "0.127": 2.7e-16, "1.0": 3e-16, "3.0": 5.7e-16, "3.141591653589793": 6.3e-11},
    "log_so3": {"rt 1e-08": 0, "rt 1e-06": 0, "rt 2e-05": 2.4e-16, "rt 0.001": 1.8e-16, "rt 0.5": 1.5e-16, "rt 1.5": 2.5e-16, "rt 3": 4.1e-15,
        "rt 3.14059": 5.6e-11, "rt 3.14157": 1.4e-07, "rt 3.14159": 0, "sin0": 0, "sinpi": 0, "out+": 0, "out-": 0},
    "sim3_exp": {"0|0": 0, "0|9.99e-06": 3.8e-17, "0|1e-05": 9.8e-12, "0|1.01e-05": 7e-12, "0|0.1": 9.3e-16, "0|1": 1.7e-16, "1e-12|0": 1.2e-16,
        "1e-12|9.99e-06": 1.2e-16, "1e-12|1e-05": 9.8e-12, "1e-12|1.01e-05": 7e-12, "1e-12|0.1": 9.6e-16, "1e-12|1": 2.2e-16, "9.999e-06|0": 1.6e-16,
        "9.999e-06|9.99e-06": 1.8e-16, "9.999e-06|1e-05": 5.2e-16, "9.999e-06|1.01e-05": 5.6e-16, "9.999e-06|0.1": 1.1e-15, "9.999e-06|1": 3.5e-16,
        "1e-05|0": 5.6e-13, "1e-05|9.99e-06": 4.8e-13, "1e-05|1e-05": 9.3e-12, "1e-05|1.01e-05": 6.7e-12, "1e-05|0.1": 1.7e-15, "1e-05|1": 3.3e-16,
        "1.0001e-05|0": 4.8e-13, "1.0001e-05|9.99e-06": 5.6e-13, "1.0001e-05|1e-05": 9.8e-12, "1.0001e-05|1.01e-05": 7.2e-12,
        "1.0001e-05|0.1": 1.3e-15, "1.0001e-05|1": 4.1e-16, "5e-05|0": 1.5e-13, "5e-05|9.99e-06": 1.7e-13, "5e-05|1e-05": 9.8e-12,
        "5e-05|1.01e-05": 7e-12, "5e-05|0.1": 1.1e-15, "5e-05|1": 3.1e-16, "0.001|0": 9e-15, "0.001|9.99e-06": 1.1e-14, "0.001|1e-05": 9.8e-12,
        "0.001|1.01e-05": 7e-12, "0.001|0.1": 1.1e-15, "0.001|1": 2.6e-16, "0.125|0": 4.7e-16, "0.125|9.99e-06": 5e-16, "0.125|1e-05": 9.8e-12,
        "0.125|1.01e-05": 7e-12, "0.125|0.1": 1.1e-15, "0.125|1": 3.1e-16, "0.127|0": 1.8e-16, "0.127|9.99e-06": 2.9e-16, "0.127|1e-05": 9.8e-12,
        "0.127|1.01e-05": 5.3e-12, "0.127|0.1": 1.1e-15, "0.127|1": 3.5e-16, "1|0": 1.8e-16, "1|9.99e-06": 1.7e-16, "1|1e-05": 9.8e-12,
        "1|1.01e-05": 7e-12, "1|0.1": 8.9e-16, "1|1": 2.5e-16, "3|0": 2e-16, "3|9.99e-06": 2.4e-16, "3|1e-05": 9.8e-12, "3|1.01e-05": 7.1e-12,
        "3|0.1": 8.9e-16, "3|1": 2.3e-16, "3.14159|0": 3.8e-16, "3.14159|9.99e-06": 3.3e-16, "3.14159|1e-05": 9.8e-12, "3.14159|1.01e-05": 7e-12,
        "3.14159|0.1": 8.3e-16, "3.14159|1": 2.7e-16},
    "R_to_q": {"0.0": 0, "1e-08": 4.2e-25, "1e-05": 1.4e-17, "1.0": 1.1e-16, "3.1405926535897932": 2.7e-16, "3.141592643589793": 2e-16,
        "3.141592653589793": 1.9e-16},
    "q_rotate_d": {"all": 5.5e-16},
    "q_rotate_f": {"all": 2.5e-07},
    "q_to_R": {"all": 2.8e-16},
    "se3_normalize": {"all": 2.3e-16},
    "se3_mul": {"all": 4.6e-16},
    "se3_map": {"all": 5.8e-16},
    "se3_from_float": {"all": 2e-16},
    "cube_rn": {"all": 1.1e-16},
    "huber": {"all": 2.6e-16},
}


def device_bound(name, label):
    return max(DEVICE_FACTOR * BOUNDS[name][str(label)], FLOOR * (2.0 ** 29 if name == "q_rotate_f" else 1.0))      # (FP32: 4 ulp of 2^-23)


# ---- small dense ---------------------------------------------------------------------------------------------------------------------------
INVERT_SIZES = (1, 2, 3, 9)       # inertial.hip:286-294 and inertial_ba.hip:150-157 call invert_n with n = 9 and 3; 1 and 2 added
CLAMP_SIZES = (9, 15)             # inertial_ba.hip:152, inertial.hip:288, inertial_optimization.hip:283 (n = 9); inertial.hip:697 (n = 15)
CLAMP_THR = 1e-12


def invert_numpy(A):
    """Gauss-Jordan with partial pivoting in float64, as invert_n does it: (ok, inverse)"""
    n = A.shape[0]
    M = np.hstack([A.astype(np.float64), np.eye(n)])
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if M[p, c] == 0.0:
            return False, None
        if p != c:
            M[[p, c]] = M[[c, p]]
        M[c] *= 1.0 / M[c, c]
        for r in range(n):
            if r != c and M[r, c] != 0.0:
                M[r] -= M[r, c] * M[c]
    return True, M[:, n:].copy()


@functools.lru_cache(maxsize=None)
def invert_cases(n):
    """list of (kind, A): 'well' random well-conditioned, 'covariance' SPD with a wide spectrum (what the product inverts), 'swap' a zero
    leading entry, 'singular' an exactly singular integer matrix (see there)"""
    rng = np.random.default_rng(0x1A7 + n)
    out = []
    for k in range(48):
        out.append(("well", rng.normal(size=(n, n)) + n * np.eye(n)))
    for k in range(16):
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        out.append(("covariance", (Q * 10.0 ** rng.uniform(-8, -2, n)) @ Q.T))
    for k in range(32):
        A = rng.normal(size=(n, n)) + n * np.eye(n)
        A[0, 0] = 0.0
        if n > 2 and k % 2:
            A[1, 1] = 0.0; A[1, 0] = 0.0                      # a second exchange further down
        if n == 1:
            A[0, 0] = 3.0
        out.append(("swap", A))
    for k in range(32):
        # exactly singular integer matrices on which the elimination itself stays exact, so that the zero pivot IS zero: a zero column
        # (0 - f 0 at every step), a zero row, and the constant matrix 2^j (the pivot row becomes exact ones, every other row exact zeros).
        # A general singular integer matrix meets 1 / 3 on its way and ends on a pivot of 1e-17, here as in any FP64 Gauss-Jordan.
        A = rng.integers(-4, 5, (n, n)).astype(np.float64)
        if k % 3 == 0:
            A[:, k % n] = 0.0
        elif k % 3 == 1:
            A[k % n, :] = 0.0
        else:
            A[:, :] = 2.0 ** (k % 5) if n > 1 else 0.0
        out.append(("singular", A))
    return out


def inverse_bound(A, X, c):
    """max |X - A^-1| a backward-stable inverse may leave: c n u k2(A) max |A^-1| (dense_probe.forward_bound's form)"""
    n = A.shape[0]
    return c * n * U * np.linalg.cond(A, 2) * np.abs(X).max()


def clamp_numpy(S, thr):
    """numpy eigh with the same clamp: eigenvalues below thr set to zero"""
    w, V = np.linalg.eigh(S)
    return (V * np.where(w < thr, 0.0, w)) @ V.T


@functools.lru_cache(maxsize=None)
def clamp_cases(n):
    """list of (kind, S, eigenvalues) with S = V diag(e) V^T"""
    rng = np.random.default_rng(0xC1A + n)
    thr = CLAMP_THR
    out = []

    def make(e, diag=False):
        e = np.array(e, np.float64)
        if diag:
            return np.diag(e)
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        S = (Q * e) @ Q.T
        return (S + S.T) / 2
    for k in range(8):
        out.append(("above", make(10.0 ** rng.uniform(-6, 2, n)), None))               # every e > thr by far: the LDL^T test passes, S untouched
        e = 10.0 ** rng.uniform(-6, 2, n); e[k % n] = thr * 10.0 ** rng.uniform(-4, -1)
        out.append(("one below", make(e), e.copy()))
        e = 10.0 ** rng.uniform(-6, 2, n); e[: 2 + k % 4] = thr * 10.0 ** rng.uniform(-4, -1, 2 + k % 4); e[0] = -1e-9 * (k % 2)
        out.append(("several below", make(e), e.copy()))
        # within 1e-12 relative of thr: the other eigenvalues stay within 10 thr, so that n u ||S|| (1e-26) is far below the 1e-24 that
        # separates the eigenvalue from thr, in S as rounded, in eigh and in any backward-stable Jacobi
        e = thr * rng.uniform(2, 10, n); e[k % n] = thr * (1 - 1e-12)
        out.append(("just below", make(e), e.copy()))
        e = thr * rng.uniform(2, 10, n); e[k % n] = thr * (1 + 1e-12)
        out.append(("just above", make(e), e.copy()))
        e = thr * rng.uniform(2, 10, n); e[k % n] = thr * (1 - 1e-12)
        out.append(("just below, diagonal", make(e, diag=True), e.copy()))
        e = thr * rng.uniform(2, 10, n); e[k % n] = thr * (1 + 1e-12)
        out.append(("just above, diagonal", make(e, diag=True), e.copy()))
        e = thr * rng.integers(2, 10, n).astype(np.float64); e[k % n] = thr
        out.append(("just above, at thr, diagonal", make(e, diag=True), e.copy()))      # e == thr exactly is kept: the clamp is `e < thr`
        e = np.repeat(10.0 ** rng.uniform(-3, 1, (n + 2) // 3), 3)[:n]; e[-1] = 0.0
        out.append(("repeated", make(e), e.copy()))
        e = 10.0 ** rng.uniform(-6, 2, n); e[k % n] = 1e-14
        out.append(("diagonal", make(e, diag=True), e.copy()))
    return out


def polar_mp(R):
    """the orthogonal polar factor of the 3 x 3 matrix R (9 floats) at 60 digits, by Newton's X <- (X + X^-T) / 2, as doubles"""
    mp = _mp()
    X = mp.matrix(3, 3)
    for k in range(9):
        X[k // 3, k % 3] = mp.mpf(float(R[k]))
    for it in range(8):             # quadratic: a perturbation of 1e-3 is below 1e-60 after seven steps
        X = (X + (X.T) ** -1) / 2
    return [float(X[k // 3, k % 3]) for k in range(9)]


def clamp_transcription(S, thr):
    """clamp_eigenvalues in float64 numpy: the LDL^T test of S - thr I, then the cyclic Jacobi with whole-row and whole-column rotations"""
    n = S.shape[0]
    A = S.astype(np.float64).copy() - thr * np.eye(n)
    pd = True
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            pd = False
            break
        for r in range(n - 1, j, -1):
            l = A[r, j] / d
            A[r, j + 1:r + 1] -= l * A[j + 1:r + 1, j]
    if pd:
        return S.copy()
    A = S.astype(np.float64).copy()
    V = np.eye(n)
    for sweep in range(60):
        diag = float((np.diag(A) ** 2).sum())
        off = float(((A - np.diag(np.diag(A))) ** 2).sum())
        if off <= 1e-30 * diag:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                a, b = A[:, p].copy(), A[:, q].copy(); A[:, p], A[:, q] = c * a - s * b, s * a + c * b
                a, b = A[p, :].copy(), A[q, :].copy(); A[p, :], A[q, :] = c * a - s * b, s * a + c * b
                a, b = V[:, p].copy(), V[:, q].copy(); V[:, p], V[:, q] = c * a - s * b, s * a + c * b
    e = np.diag(A).copy()
    e[e < thr] = 0.0
    return (V * e) @ V.T


def clamp_figure(S, out, thr):
    """max |out - eigh clamp| in units of n u ||S||_2"""
    n = S.shape[0]
    return np.abs(out - clamp_numpy(S, thr)).max() / (n * U * np.linalg.norm(S, 2))


def inverse_mp(A):
    """the inverse at 60 digits, rounded to double"""
    mp = _mp()
    X = mp.matrix(A.tolist()) ** -1
    return np.array([[float(X[i, j]) for j in range(A.shape[0])] for i in range(A.shape[0])])


def inverse_figure(A, X):
    """max |X - A^-1| in units of n u k2(A) max |A^-1|"""
    Xr = inverse_mp(A)
    return np.abs(X - Xr).max() / (A.shape[0] * U * np.linalg.cond(A, 2) * np.abs(Xr).max())


def jacobi_numpy(A, skip_pair=None):
    """row_jacobi.h's g_jacobi in float64 numpy: (eigenvalues = the diagonal left, V).  Same pair order, skipped rotations and stopping rule."""
    A = A.astype(np.float64).copy()
    m = A.shape[0]
    V = np.eye(m)
    with np.errstate(over="ignore", under="ignore"):
        fro = float(sum((A[:, j] ** 2).sum() for j in range(m)))
    back = 0
    if not (2.0 ** -600 <= fro <= 2.0 ** 600):                 # the exact power-of-two rescale of matrices whose squares leave FP64's range
        mx = float(np.abs(A).max())
        if 0 < mx < math.inf:
            back = math.frexp(mx)[1]
            A = np.ldexp(A, -back)
            fro = float(sum((A[:, j] ** 2).sum() for j in range(m)))
    for sweep in range(30):
        off = float(sum((A[:j, j] ** 2).sum() for j in range(m)))
        if not off > 1e-30 * fro:
            break
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq = A[p, q]
                if apq == 0.0 or (p, q) == skip_pair:
                    continue
                app, aqq = A[p, p], A[q, q]
                theta = (aqq - app) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                akp, akq = A[:, p].copy(), A[:, q].copy()
                np_, nq = c * akp - s * akq, s * akp + c * akq
                mid = np.ones(m, bool); mid[[p, q]] = False
                A[mid, p] = np_[mid]; A[p, mid] = np_[mid]; A[mid, q] = nq[mid]; A[q, mid] = nq[mid]
                vkp, vkq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vkp - s * vkq, s * vkp + c * vkq
                A[p, p], A[q, q], A[p, q], A[q, p] = app - t * apq, aqq + t * apq, 0.0, 0.0
    return np.ldexp(np.diag(A).copy(), back), V


JACOBI_SIZES = (3, 9, 12, 16)
JACOBI_KINDS = ("spd", "rank m-1", "rank m-2", "repeated", "diagonal", "zero", "scaled 1e-300", "scaled 1e+150")


@functools.lru_cache(maxsize=None)
def jacobi_case(m, kind, k):
    rng = np.random.default_rng(0x7AC + 100 * m + k)
    if kind == "spd":
        G = rng.normal(size=(m, m + 4)); return G @ G.T
    if kind in ("rank m-1", "rank m-2"):
        r = m - 1 if kind == "rank m-1" else m - 2
        G = rng.normal(size=(r, m)); return G.T @ G          # the Gram matrix of r < m rows (two_view.hip, mlpnp_solver.hip)
    if kind == "repeated":
        Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
        H = np.eye(m) - 2 * np.outer(Q[:, 0], Q[:, 0])        # a Householder reflection: eigenvalues exactly -1 and 1 (m - 1 times)
        return (H + H.T) / 2 * 4.0
    if kind == "diagonal":
        return np.diag(rng.uniform(-3, 3, m))
    if kind == "zero":
        return np.zeros((m, m))
    G = rng.normal(size=(m, m + 4))
    return (G @ G.T) * (1e-300 if kind == "scaled 1e-300" else 1e150)


def jacobi_check(A, w, V):
    """the four figures of one eigen-decomposition against numpy eigh, each in units of m u ||A||_2 (angle: m u ||A|| / gap)"""
    m = A.shape[0]
    wr, Vr = np.linalg.eigh(A)
    nrm = np.abs(wr).max()
    unit = m * U * nrm if nrm > 0 else 1.0
    order = np.argsort(w)
    fig = {"eig": np.abs(w[order] - wr).max() / unit,
           "res": np.linalg.norm(A @ V - V * w, 2) / unit,
           "orth": np.linalg.norm(V.T @ V - np.eye(m), 2) / (m * U)}
    null = np.abs(wr) <= 64 * m * U * nrm
    if 0 < null.sum() < m and nrm > 0:
        gap = np.abs(wr[~null]).min()
        N, Nr = V[:, order][:, null], Vr[:, null]
        fig["null"] = np.linalg.norm(N - Nr @ (Nr.T @ N), 2) / (m * U * nrm / gap)      # sine of the largest angle between the null spaces
    return fig


# c of the backward-stability bounds c n u ||A|| (eigenvalues, residual; orthogonality: c n u; null space: c n u ||A|| / gap) and
# c n u k(A) max |A^-1| (inverses): the largest figure of the FP64 numpy transcription over the same inputs, times 8, rounded up.
# test_device_math_cpu.py measures the figures again.
C_JACOBI = 28.0     # measured: orthogonality 3.50 (scaled 1e+150, m = 16), eigenvalues 2.67, null space 1.84, residual 1.44
C_CLAMP = 37.0      # measured: 4.52 (an eigenvalue 1e-12 relative below thr, n = 9)
C_INVERT = 6.3      # measured: 0.783 (n = 2, well-conditioned)


# ---- wave.h: the scan as the header writes it ---------------------------------------------------------------------------------------------
def dpp_bruteforce(v, op, ident):
    """Per-lane simulation of the six DPP steps of MORB_DPP_SCAN on 64 lanes, then the read of lane 63.  row_shr:n: lane i reads lane
    i - n of its own row of 16, or keeps `ident` (bound_ctrl off) when that falls out of the row; row_bcast:15 with row mask 0xa: the lanes
    of rows 1 and 3 read lane 15 of the row before, rows 0 and 2 are masked and keep `ident`; row_bcast:31 with row mask 0xc: rows 2 and 3 read
    lane 31.  Every lane then applies op(own, read)."""
    v = list(v)
    assert len(v) == 64
    for sh in (1, 2, 4, 8):
        v = [op(v[i], v[i - sh] if (i % 16) >= sh else ident) for i in range(64)]
    v = [op(v[i], v[(i // 16) * 16 - 1] if (i // 16) in (1, 3) else ident) for i in range(64)]
    v = [op(v[i], v[31] if (i // 16) in (2, 3) else ident) for i in range(64)]
    return v[63]


def _row_tree(r):
    """lane 15 of a row after row_shr 1, 2, 4, 8: a balanced tree over the 16 lanes, the HIGHER lane the left operand at every node"""
    r = list(r)
    while len(r) > 1:
        r = [r[k + 1] + r[k] for k in range(0, len(r), 2)]
    return r[0]


def sum_f64_model(v):
    """The order of morbwave::sum_f64: T_r = the tree of row r; lane 63 = (T3 + T2) + (T1 + T0).  (The identity a masked or out-of-row
    lane adds never reaches lane 63: every value on its path was read before the step that would have touched it.)"""
    v = [float(x) for x in v]
    T = [_row_tree(v[16 * r: 16 * r + 16]) for r in range(4)]
    return (T[3] + T[2]) + (T[1] + T[0])


def row_sum_f64_model(v):
    """morbwave::row_sum_f64: every lane of row r receives T_r"""
    v = [float(x) for x in v]
    return [_row_tree(v[16 * (i // 16): 16 * (i // 16) + 16]) for i in range(64)]


def wave_call(op, x, threads, src=0):
    """probe_wave over x (a multiple of `threads` values): op 0 min_u32, 1 sum_i32, 2 min_u64, 3 sum_f64, 4 row_sum_f64, 5 readlane_f64"""
    import torch
    x = np.ascontiguousarray(x)
    assert x.size % threads == 0
    dx = torch.from_numpy(x.view(np.uint8)).cuda()
    dout = torch.zeros_like(dx)
    torch.cuda.synchronize()
    st = lib().probe_wave(op, dx.data_ptr(), dout.data_ptr(), x.size // threads, threads, src)
    assert st == 0, (op, st)
    return dout.cpu().numpy().view(x.dtype)


def ransac_call(nt, flags):
    """probe_ransac_block: (block_count, the compaction's running total, the kept indices in slot order)"""
    import torch
    n = len(flags)
    df = torch.from_numpy(np.ascontiguousarray(np.concatenate([flags, [0]]).astype(np.int32))).cuda()
    cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = lib().probe_ransac_block(nt, df.data_ptr(), n, cnt.data_ptr(), kept.data_ptr())
    assert st == 0, (nt, n, st)
    c = cnt.cpu().numpy()
    return int(c[0]), int(c[1]), kept.cpu().numpy()[:n]


RANSAC_BLOCKS = (256,)     # SS_NT (sim3_solver.hip:33), MORB_MLPNP_THREADS (mlpnp_solver.hip:31), MORB_TWO_VIEW_THREADS (two_view.hip:44): all 256
RANSAC_BLOCKS_ALT = (64, 128)   # the documented -DMORB_MLPNP_THREADS=128 / 64 and -DMORB_TWO_VIEW_THREADS=128 builds


def spread_doubles(rng):
    """64 doubles spanning 2^0 .. 2^-60 with full mantissas and both signs: the order of a sum changes its last bits"""
    return rng.uniform(1, 2, 64) * 2.0 ** -rng.integers(0, 61, 64).astype(np.float64) * rng.choice([-1.0, 1.0], 64)
