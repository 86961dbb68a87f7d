"""The scalar, 3 x 3 and wave-level device functions under every optimiser and solver, each launched ALONE through
tests/native/libmath_probe.so (tests/native/math_probe_*.hip) and compared with a plain reference of the same operation:
  * the libm restatements (csrc/libm_f32.h, libm_f64.h, sin_glibc_small) and include/morb/camera_math.h: the gfx950 compile against the
    x86-64 compile of the same header text, bit for bit (test_device_math_cpu.py pins that host build to this project's libm);
  * the SE3 / SO3 / Sim3 algebra with every threshold branch, against the reference project's formula at 60 digits (math_probe.py);
  * invert_n, clamp_eigenvalues, normalize_rotation_f and the row Jacobi against numpy / mpmath within backward-stability bounds;
  * the DPP reductions of csrc/wave.h and the compaction of csrc/ransac_block.h, exact — the order of sum_f64 included.
The whole-optimiser tests run clean synthetic scenes with LM steps of 1e-3 rad: they enter the common branch of each of these only.
Bounds: math_probe.py (BOUNDS and the C_* constants), measured on FP64 transcriptions by test_device_math_cpu.py, never on the device."""
import math

import numpy as np
import pytest

import math_probe as P

pytestmark = pytest.mark.gpu


def _assert_bits(name, x, dev, ref, what="host"):
    ok = P.same_bits(dev, ref)
    if ok.ndim > 1:
        ok = ok.all(axis=1)
    bad = np.flatnonzero(~ok)
    print(f"{name}: {len(ok)} inputs, {len(bad)} differ from the {what} build")
    assert len(bad) == 0, (name, x[bad[:5]], dev[bad[:5]], ref[bad[:5]])


# ---- libm on the device, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["atanf", "acosf", "tanf", "sinf", "cosf"])
def test_libm_f32_bits(name):
    """every 257th float, +-2048 neighbours of every literal of the function, every 1024th denormal, +-0, +-inf, NaNs.  sinf / cosf: cut to
    |y| < 120, the range libm_f32.h restates them for — beyond it `(int32_t)r` overflows, which C++ leaves undefined and the two
    compilers resolve differently (x86-64: INT_MIN, gfx950: saturation)."""
    x = P.f32_inputs(name)
    _assert_bits(name, x.view(np.float32), P.device(name, x)[:, 0], P.host(name, x)[:, 0])


def test_libm_atan2f_bits():
    yx = P.atan2f_inputs()
    _assert_bits("atan2f", yx.view(np.float32), P.device("atan2f", yx)[:, 0], P.host("atan2f", yx)[:, 0])


@pytest.mark.parametrize("name", ["sin64", "cos64", "sincos64", "exp64"])
def test_libm_f64_bits(name):
    x = P.f64_exp_inputs() if name == "exp64" else P.f64_sincos_inputs()
    _assert_bits(name, x, P.device(name, x), P.host(name, x))


def test_sin_glibc_small_is_sin_glibc():
    """optimizer_device.h's third copy of glibc's small-argument sin: the bits of libm_f64.h's sin_glibc for |x| < 0.126; from 0.126 on it is
    the device library's sin, held to the 4 ulp of the OpenCL full profile plus glibc's own 0.55"""
    x = P.sin_small_inputs()
    dev = P.device("sin_small", x)[:, 0]
    ref = P.host("sin64", x)[:, 0]
    inside = np.abs(x) < 0.126
    assert inside.sum() > 4_000_000 and (~inside).sum() >= 2048
    _assert_bits("sin_glibc_small", x[inside], dev[inside], ref[inside])
    _assert_bits("sin_glibc_small vs the device's sin_glibc", x[inside], dev[inside], P.device("sin64", x[inside])[:, 0], "device")
    ulps = P.ulp_diff(dev[~inside], ref[~inside]).max()
    print("beyond 0.126:", ulps, "ulp")
    assert ulps <= 5


# ---- camera_math.h ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam", [("pinhole_project", "PINHOLE"), ("kb8_project", "KB8"), ("kb8_project", "KB8_B")])
def test_camera_project_bits(name, cam):
    rec = P.cam_records(getattr(P, cam), P.camera_points(name.startswith("kb8")), np.float32)
    _assert_bits(name, rec[:, 8:], P.device(name, rec), P.host(name, rec))


@pytest.mark.parametrize("name,cam", [("pinhole_unproject", "PINHOLE"), ("kb8_unproject", "KB8"), ("kb8_unproject", "KB8_B")])
def test_camera_unproject_bits(name, cam):
    rec = P.cam_records(getattr(P, cam), P.camera_pixels(), np.float32)
    _assert_bits(name, rec[:, 8:], P.device(name, rec), P.host(name, rec))


def _kb8_theta_float(Pn):
    """theta of kb8_project_d as the header computes it: atan2f of the float-rounded operands (the host entry of the restated atan2f)"""
    r = np.sqrt((Pn[:, 0] * Pn[:, 0] + Pn[:, 1] * Pn[:, 1]).astype(np.float32))
    return P.host("atan2f", np.column_stack([r, Pn[:, 2].astype(np.float32)]).astype(np.float32))[:, 0].astype(np.float64)


@pytest.mark.parametrize("cam", ["KB8", "KB8_B"])
def test_kb8_project_d(cam):
    """Not bit-equal by construction: kb8_project_d calls cos(psi) and sin(psi) of a double, the device library's on the GPU and the host
    libm's in the host entry.  u = fl(fl(fx r cos) + cx): a cosine within 4 ulp (OpenCL full profile) against one within 1 ulp moves the
    product by <= 5 eps |fx r|, the two roundings add <= eps (|fx r| + |cx|): |u_dev - u_host| <= 8 eps (|fx r| + |cx|), and so for v."""
    c = getattr(P, cam).astype(np.float64)
    Pn = P.camera_points(True)
    rec = P.cam_records(getattr(P, cam), Pn, np.float64)
    dev, ref = P.device("kb8_project_d", rec), P.host("kb8_project_d", rec)
    th = _kb8_theta_float(Pn)
    r = np.abs(th + c[4] * th ** 3 + c[5] * th ** 5 + c[6] * th ** 7 + c[7] * th ** 9)
    bound = 8 * P.EPS * np.column_stack([c[0] * r + abs(c[2]), c[1] * r + abs(c[3])])
    ratio = np.abs(dev - ref) / bound
    print(f"kb8_project_d {cam}: largest |dev - host| / bound {ratio.max():.3g}; bit-equal {P.same_bits(dev, ref).mean():.4f}")
    assert np.isfinite(ref).all() and (ratio <= 1).all()


@pytest.mark.parametrize("cam", ["KB8", "KB8_B"])
def test_kb8_project_jac(cam):
    """Not bit-equal by construction: kb8_project_jac calls atan2 of doubles (6 ulp in the OpenCL full profile, 1 ulp on the host).  theta
    enters f and fd, whose relative sensitivity to theta is amp = max(1, theta |fd / f|, theta |fd' / fd|), so f and fd differ by
    <= 7 amp eps relatively; every entry is a sum of at most two terms of <= 10 operations: |J_dev - J_host| <= (7 amp + 16) eps sum |terms|.
    On the optical axis (r = 0) every entry is 0 / 0 on both sides."""
    c = getattr(P, cam).astype(np.float64)
    Pn = P.camera_points(True)
    rec = P.cam_records(getattr(P, cam), Pn, np.float64)
    dev, ref = P.device("kb8_project_jac", rec), P.host("kb8_project_jac", rec)
    x, y, z = Pn.T
    with np.errstate(all="ignore"):
        x2, y2, z2 = x * x, y * y, z * z
        r2 = x2 + y2
        r = np.sqrt(r2)
        r3 = r2 * r
        th = np.arctan2(r, z)
        f = th + th ** 3 * c[4] + th ** 5 * c[5] + th ** 7 * c[6] + th ** 9 * c[7]
        fd = 1 + 3 * c[4] * th ** 2 + 5 * c[5] * th ** 4 + 7 * c[6] * th ** 6 + 9 * c[7] * th ** 8
        fdd = 6 * c[4] * th + 20 * c[5] * th ** 3 + 42 * c[6] * th ** 5 + 72 * c[7] * th ** 7
        amp = np.maximum(1, np.maximum(np.abs(th * fd / f), np.abs(th * fdd / fd)))
        a, b = np.abs(fd * z / (r2 * (r2 + z2))), np.abs(f / r3)
        terms = np.column_stack([c[0] * (a * x2 + b * y2), c[0] * (a + b) * np.abs(x * y), c[0] * np.abs(fd * x / (r2 + z2)),
                                 c[1] * (a + b) * np.abs(x * y), c[1] * (a * y2 + b * x2), c[1] * np.abs(fd * y / (r2 + z2))])
        bound = ((7 * amp + 16) * P.EPS)[:, None] * terms
    axis = r2 == 0
    assert axis.sum() >= 512 and (np.isnan(dev[axis]) == np.isnan(ref[axis])).all()
    ok = ~axis & np.isfinite(bound).all(axis=1)
    assert ok.sum() > 0.99 * len(ok)
    diff = np.abs(dev[ok] - ref[ok])
    with np.errstate(all="ignore"):
        ratio = np.nanmax(np.where(bound[ok] > 0, diff / bound[ok], 0.0))
    print(f"kb8_project_jac {cam}: largest |dev - host| / bound {ratio:.3g}; bit-equal {P.same_bits(dev[ok], ref[ok]).mean():.4f}")
    assert (diff <= bound[ok]).all()


# ---- SE3 / SO3 / Sim3 --------------------------------------------------------------------------------------------------------------------------
def _held(name, out, probe=None):
    """every input class of `name` within its bound; returns the per-class table"""
    err = P.class_errors(name, out)
    table = {l: (e, P.device_bound(name, l)) for l, e in err.items()}
    for l, (e, b) in table.items():
        print(f"{probe or name} [{l}]: error {e:.3g} bound {b:.3g}")
    bad = {l: v for l, v in table.items() if not v[0] <= v[1]}
    assert not bad, (probe or name, bad)
    return table


@pytest.mark.parametrize("name", P.ALGEBRA)
def test_algebra(name):
    """q_rotate<float / double>, q_to_R, se3_normalize, se3_mul, se3_map, se3_from_float, cube_rn, huber against 60 digits"""
    lab, x, ref, tr, br, groups = P.lie_case(name)
    out = P.device(name, x)
    _held(name, out)
    if name == "huber":
        # e == delta^2 exactly and one ulp either side: inside, rho is e and w is 1, bit for bit; the first e beyond takes the sqrt branch
        d2 = x[:, 0] * x[:, 0]
        inside = x[:, 1] <= d2
        assert (x[:, 1] == d2).sum() >= len(P.HUBER_DELTAS) and (x[:, 1] == np.nextafter(d2, np.inf)).sum() >= len(P.HUBER_DELTAS)
        assert P.same_bits(out[inside, 0], x[inside, 1]).all() and (out[inside, 1] == 1.0).all()
        assert (out[~inside, 1] <= 1.0).all()
    if name == "cube_rn":
        # rounded once: within half an ulp of x^3 (plus the double rounding the header allows for)
        mp = P._mp()
        ulps = max(abs(mp.mpf(float(o)) - r[0]) / mp.mpf(float(np.spacing(o))) for o, r in zip(out[:, 0], ref) if o != 0)
        print("cube_rn: largest error", float(ulps), "ulp")
        assert ulps <= 0.5 + 2.0 ** -10


def test_R_to_q_both_headers():
    """optimizer_device.h's constant-index R_to_q_case<I, J, K> and sim3_math.h's run-time index form: identical bits, the quaternion of the
    60-digit formula up to sign, unit norm to 4 ulp; all four branches entered >= 100 times"""
    lab, x, ref, tr, br, groups = P.lie_case("R_to_q")
    counts = np.bincount(br, minlength=4)
    print("R_to_q inputs per branch (trace > 0, largest diagonal x, y, z):", counts.tolist())
    assert (counts >= 100).all()
    a, b = P.device("R_to_q_se3", x), P.device("R_to_q_sim3", x)
    _assert_bits("R_to_q: optimizer_device.h vs sim3_math.h", x, a, b, "sim3_math.h")
    _held("R_to_q", a, "R_to_q_se3")
    norm = np.abs(np.sqrt((a * a).sum(axis=1)) - 1).max()
    print("largest | |q| - 1 |:", norm / P.EPS, "ulp")
    assert norm <= 4 * P.EPS


@pytest.mark.parametrize("name", ["se3_exp", "exp_so3", "sim3_exp", "log_so3", "right_jacobian_so3", "inv_right_jacobian_so3"])
def test_lie_branches(name):
    """the theta (and sigma) ladder over random axes, every threshold branch counted, against the reference's formula at 60 digits"""
    lab, x, ref, tr, br, groups = P.lie_case(name)
    counts = np.bincount(br)
    print(f"{name} inputs per branch:", counts.tolist())
    assert len(counts) == {"sim3_exp": 4, "log_so3": 3}.get(name, 2) and (counts >= 100).all()
    out = P.device(name, x)
    assert np.isfinite(out).all()
    _held(name, out)
    if name == "log_so3":
        early = br > 0            # the early returns hand back the antisymmetric part untouched: exact
        w0 = np.column_stack([(x[:, 7] - x[:, 5]) / 2, (x[:, 2] - x[:, 6]) / 2, (x[:, 3] - x[:, 1]) / 2])
        assert P.same_bits(out[early], w0[early]).all()
    if name in ("right_jacobian_so3", "inv_right_jacobian_so3"):
        eye = np.eye(3).ravel()
        assert P.same_bits(out[br == 1], np.broadcast_to(eye, out[br == 1].shape)).all()       # d < 1e-5: the identity, exactly


def test_right_jacobian_times_its_inverse():
    """Jr Jr^-1 = I over the ladder.  Each factor is within its class bound b of the formula, and the formulas are exact inverses of each
    other for d >= 1e-5, so |Jr Jr^-1 - I| <= 3 max|Jr| max|Jr^-1| (b_r + b_inv + 4 eps) entrywise, the 3 from the row sums."""
    lab, x, *_ = P.lie_case("right_jacobian_so3")
    Jr = P.device("right_jacobian_so3", x).reshape(-1, 3, 3)
    Ji = P.device("inv_right_jacobian_so3", x).reshape(-1, 3, 3)
    prod = Jr @ Ji
    for l in dict.fromkeys(lab.tolist()):
        m = lab == l
        err = np.abs(prod[m] - np.eye(3)).max(axis=(1, 2))
        tol = 3 * np.abs(Jr[m]).max(axis=(1, 2)) * np.abs(Ji[m]).max(axis=(1, 2)) * \
            (P.device_bound("right_jacobian_so3", l) + P.device_bound("inv_right_jacobian_so3", l) + 4 * P.EPS)
        print(f"Jr Jr^-1 [{l}]: error {err.max():.3g} tolerance {tol.min():.3g}")
        assert (err <= tol).all(), l


def test_sim3_group_laws():
    """S S^-1 acts as the identity on points, and (A B) x = A (B x).  Every step is a handful of FP64 operations on quantities no larger
    than s |x| + |t|: 64 eps of that sum (for the composition: of the sizes of both maps)."""
    rng = np.random.default_rng(0x5173)
    n = 4096

    def sims(k):
        q = rng.normal(size=(k, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        return np.column_stack([q, rng.uniform(-1, 1, (k, 3)) * 10.0 ** rng.uniform(-2, 2, (k, 1)), 10.0 ** rng.uniform(-2, 2, k)])
    A, B = sims(n), sims(n)
    X = rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    nx, ta, tb = np.linalg.norm(X, axis=1), np.linalg.norm(A[:, 4:7], axis=1), np.linalg.norm(B[:, 4:7], axis=1)
    back = P.device("sim3_roundtrip", np.column_stack([A, X]))
    err = np.abs(back - X).max(axis=1) / (64 * P.EPS * (nx + 2 * ta))
    print("S S^-1 x - x: largest error / tolerance", err.max())
    assert (err <= 1).all()
    AB = P.device("sim3_mul", np.column_stack([A, B]))
    lhs = P.device("sim3_map", np.column_stack([AB, X]))
    rhs = P.device("sim3_map", np.column_stack([A, P.device("sim3_map", np.column_stack([B, X]))]))
    err = np.abs(lhs - rhs).max(axis=1) / (64 * P.EPS * (A[:, 7] * (B[:, 7] * nx + tb) + ta))
    print("(A B) x - A (B x): largest error / tolerance", err.max())
    assert (err <= 1).all()
    assert P.same_bits(AB[:, 7], A[:, 7] * B[:, 7]).all()
    inv = P.device("sim3_inverse", A)
    assert P.same_bits(inv[:, :3], -A[:, :3]).all() and P.same_bits(inv[:, 3], A[:, 3]).all() and P.same_bits(inv[:, 7], 1.0 / A[:, 7]).all()


# ---- small dense -------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", P.INVERT_SIZES)
def test_invert_n(n):
    """Gauss-Jordan with partial pivoting at the product's n (9, 3) and at 1, 2: well-conditioned and covariance-like matrices and ones
    whose zero leading entry forces a row exchange, within C_INVERT n u k(A) max |A^-1| of the 60-digit inverse; exactly singular integer
    matrices return false"""
    import torch
    cases = P.invert_cases(n)
    A = np.array([c[1] for c in cases])
    dA = _dev(A)
    dX = torch.full_like(dA, float("nan"))
    dM = torch.zeros((len(cases), 2 * n * n), dtype=torch.float64, device="cuda")
    ok = torch.full((len(cases),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert P.lib().probe_invert_n(dA.data_ptr(), n, len(cases), dX.data_ptr(), dM.data_ptr(), ok.data_ptr()) == 0
    ok, X = ok.cpu().numpy(), dX.cpu().numpy()
    worst = {}
    for i, (kind, Ai) in enumerate(cases):
        assert ok[i] == (0 if kind == "singular" else 1), (n, i, kind)
        if kind == "singular":
            assert np.isnan(X[i]).all()                 # nothing written
            continue
        worst[kind] = max(worst.get(kind, 0.0), P.inverse_figure(Ai, X[i]))
    print(f"invert_n n = {n}: largest error / (n u k |A^-1|) per kind {worst}; allowed {P.C_INVERT}")
    assert max(worst.values()) <= P.C_INVERT
    assert (dA.cpu().numpy() == A).all()


@pytest.mark.parametrize("n", P.CLAMP_SIZES)
def test_clamp_eigenvalues(n):
    """S = V diag(e) V^T at the product's n (9, 15) and threshold: every e above thr (also by 1e-12 relative) keeps every input byte; one,
    several, repeated, diagonal and just-below eigenvalues under thr go through the cyclic-Jacobi rebuild, within C_CLAMP n u ||S|| of
    numpy eigh with the same clamp"""
    import torch
    cases = P.clamp_cases(n)
    S = np.array([c[1] for c in cases])
    dS = _dev(S)
    dA, dV = torch.zeros_like(dS), torch.zeros_like(dS)
    torch.cuda.synchronize()
    assert P.lib().probe_clamp_eigenvalues(dS.data_ptr(), n, P.CLAMP_THR, len(cases), dA.data_ptr(), dV.data_ptr()) == 0
    out = dS.cpu().numpy()
    worst = {}
    for i, (kind, Si, e) in enumerate(cases):
        if kind.split(",")[0] in ("above", "just above"):
            assert out[i].tobytes() == Si.tobytes(), (n, i, kind)
            continue
        assert out[i].tobytes() != Si.tobytes(), (n, i, kind)
        worst[kind] = max(worst.get(kind, 0.0), P.clamp_figure(Si, out[i], P.CLAMP_THR))
    print(f"clamp_eigenvalues n = {n}: largest error / (n u ||S||) per kind {worst}; allowed {P.C_CLAMP}")
    assert max(worst.values()) <= P.C_CLAMP


def test_normalize_rotation_f():
    """rotations perturbed by 1e-7 .. 1e-3 per entry against the FP64 polar factor rounded to float: numpy's U V^T of the SVD, and — since
    LAPACK's own error is of the size of the difference looked for — the polar factor at 60 digits, which the SVD must agree with to
    1e-13.  Three Newton steps from 1e-3 leave 1e-24: the FP64 iterate is the polar factor up to the rounding of its LAST step (the
    earlier ones are squared away), <= 30 operations on entries <= 1 in an entry's data path, 32 u = 2^-48.  The float rounding then
    lands on the reference's float or, when a rounding boundary lies within that distance, on its neighbour:
    |out - ref| <= ulp_float(ref) + 2^-48 entry by entry, and out is orthogonal to 4 float ulp."""
    rng = np.random.default_rng(0x2071)
    n = 384
    ax = rng.normal(size=(n, 3))
    ax *= (rng.uniform(0, math.pi, n) / np.linalg.norm(ax, axis=1))[:, None]
    R = np.array([P.exp_so3(list(a), P.F64)[0] for a in ax])
    R[:16] = np.eye(3).ravel()
    Rp = (R + rng.uniform(-1, 1, (n, 9)) * 10.0 ** rng.uniform(-7, -3, (n, 1))).astype(np.float32)
    out = P.device("normalize_rotation_f", Rp)
    ref64 = np.array([P.polar_mp(r) for r in Rp])
    Uu, _, Vt = np.linalg.svd(Rp.astype(np.float64).reshape(n, 3, 3))
    assert np.abs((Uu @ Vt).reshape(n, 9) - ref64).max() <= 1e-13
    ref = ref64.astype(np.float32)
    diff = np.abs(out.astype(np.float64) - ref64)
    tol = 0.5 * np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -48       # (against the unrounded reference: half a float ulp, plus the slop)
    print(f"normalize_rotation_f: largest difference / tolerance {(diff / tol).max():.3g}, bit-equal entries {P.same_bits(out, ref).mean():.6f}")
    assert (diff <= tol).all()
    o = out.astype(np.float64).reshape(n, 3, 3)
    assert np.abs(o @ o.transpose(0, 2, 1) - np.eye(3)).max() <= 4 * 2.0 ** -23


# ---- row Jacobi --------------------------------------------------------------------------------------------------------------------------------
def _row_jacobi(mats):
    """four m x m matrices on the four rows of one wave: (eigenvalues (4, m), eigenvectors (4, m, m))"""
    import torch
    m = mats[0].shape[0]
    dA = _dev(np.array(mats))
    W = torch.full((4, m), float("nan"), dtype=torch.float64, device="cuda")
    V = torch.full((4, m, m), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert P.lib().probe_row_jacobi(dA.data_ptr(), m, W.data_ptr(), V.data_ptr()) == 0
    return W.cpu().numpy(), V.cpu().numpy()


@pytest.mark.parametrize("m", P.JACOBI_SIZES)
def test_row_jacobi(m):
    """g_jacobi at m = 3, 9, 12, 16 (= ROW_LANES): one wave carrying four different matrices on its four rows of 16 lanes, and the same
    matrices one per launch (the other rows idle on zero matrices) with identical bits.  Eigenvalues, ||A V - V L||, ||V^T V - I|| and the
    null space of the rank-deficient Gram matrices against numpy eigh, each within C_JACOBI m u ||A|| (null space: / gap).
    The 1e-300-scaled matrix is the one that found the underflow of the stopping rule's squares (row_jacobi.h: the power-of-two rescale):
    without it the squares are all zero, the loop stops before its first rotation and V = I comes back (the numpy transcription of that
    rule: 1e15 bounds out)."""
    kinds = P.JACOBI_KINDS
    worst = {}
    for g in range(0, len(kinds), 4):
        for k in range(2):
            mats = [P.jacobi_case(m, kinds[(g + r) % len(kinds)], k) for r in range(4)]
            W, V = _row_jacobi(mats)
            for r in range(4):
                alone = [np.zeros((m, m))] * 4
                alone[r] = mats[r]
                W1, V1 = _row_jacobi(alone)
                assert W1[r].tobytes() == W[r].tobytes() and V1[r].tobytes() == V[r].tobytes(), (m, kinds[(g + r) % len(kinds)], r)
                fig = P.jacobi_check(mats[r], W[r], V[r])
                kind = kinds[(g + r) % len(kinds)]
                if kind.startswith("rank"):
                    assert "null" in fig
                for key, v in fig.items():
                    worst[(kind, key)] = max(worst.get((kind, key), 0.0), v)
    print(f"g_jacobi m = {m}: figures in units of m u ||A|| {worst}; allowed {P.C_JACOBI}")
    bad = {k: v for k, v in worst.items() if not v <= P.C_JACOBI}
    assert not bad, bad


# ---- wave.h and ransac_block.h ---------------------------------------------------------------------------------------------------------------
def _wave_sets_u32(rng, threads):
    sets = [rng.integers(0, 2 ** 32, threads, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    sets.append(np.full(threads, 12345, np.uint32))                                                    # all equal
    for pos in (0, 63):                                                                                # the extreme in lane 0 / lane 63
        v = rng.integers(1000, 2 ** 32, threads, dtype=np.uint64).astype(np.uint32)
        v[pos::64] = np.arange(threads // 64, dtype=np.uint32) + 1
        sets.append(v)
    sets.append(np.full(threads, 0xFFFFFFFF, np.uint32))
    return sets


@pytest.mark.parametrize("threads", [64, 256])
def test_wave_integer_reductions(threads):
    """min_u32, sum_i32, min_u64 on one wave and on a 256-thread block (four waves with different data): every lane receives its own
    wave's result, exactly"""
    rng = np.random.default_rng(0x3A7E + threads)
    for v in _wave_sets_u32(rng, threads):
        got = P.wave_call(0, v, threads)
        assert (got.reshape(-1, 64) == v.reshape(-1, 64).min(axis=1)[:, None]).all()
        iv = (v >> 8).astype(np.int32) - (1 << 22)
        got = P.wave_call(1, iv, threads)
        assert (got.reshape(-1, 64) == iv.reshape(-1, 64).sum(axis=1, dtype=np.int64).astype(np.int32)[:, None]).all()
    sets64 = [rng.integers(0, 2 ** 63, threads, dtype=np.uint64) * 2 + 1 for _ in range(3)]
    ties = (rng.integers(0, 3, threads, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 2 ** 32, threads, dtype=np.uint64)   # ties in the high word
    sets64 += [ties, np.full(threads, 7 << 32, np.uint64), ties[::-1].copy()]
    for pos in (0, 63):
        v = ties.copy() + (np.uint64(5) << np.uint64(32))
        v[pos::64] = (np.uint64(5) << np.uint64(32)) | np.uint64(3)
        sets64.append(v)
    for v in sets64:
        got = P.wave_call(2, v, threads)
        assert (got.reshape(-1, 64) == v.reshape(-1, 64).min(axis=1)[:, None]).all()


@pytest.mark.parametrize("threads", [64, 256])
def test_wave_sum_f64_order(threads):
    """sum_f64 and row_sum_f64 return the bits of the scan as wave.h writes it (math_probe.sum_f64_model — the order is part of the bit-exact
    contract with the oracle): on integer-valued doubles, where every order agrees, and on doubles spanning 2^0 .. 2^-60, where a plain
    left-to-right sum differs from the model (asserted first, so the set discriminates)"""
    rng = np.random.default_rng(0x5CA)
    for trial in range(8):
        ints = rng.integers(-2 ** 40, 2 ** 40, threads).astype(np.float64)
        spread = np.concatenate([P.spread_doubles(rng) for _ in range(threads // 64)])
        for kind, v in (("integers", ints), ("spread", spread)):
            waves = v.reshape(-1, 64)
            model = np.array([P.sum_f64_model(w) for w in waves])
            left = np.array([np.add.accumulate(w)[-1] for w in waves])                 # (accumulate adds strictly left to right)
            if kind == "spread" and trial < 4:
                assert (left != model).any(), "the set does not tell the orders apart"
            if kind == "integers":
                assert (left == model).all()
            got = P.wave_call(3, v, threads).reshape(-1, 64)
            assert P.same_bits(got, np.broadcast_to(model[:, None], got.shape)).all(), (kind, trial)
            rows = np.array([P.row_sum_f64_model(w) for w in waves])
            got = P.wave_call(4, v, threads).reshape(-1, 64)
            assert P.same_bits(got, rows).all(), (kind, trial)


@pytest.mark.parametrize("threads", [64, 256])
def test_wave_readlane_f64(threads):
    rng = np.random.default_rng(0x4EAD)
    v = rng.normal(size=threads) * 10.0 ** rng.uniform(-300, 300, threads)
    v[5] = -0.0
    for src in (0, 15, 16, 31, 32, 63):
        got = P.wave_call(5, v, threads, src).reshape(-1, 64)
        assert P.same_bits(got, np.broadcast_to(v.reshape(-1, 64)[:, src][:, None], got.shape)).all(), src
    assert P.lib().probe_wave(5, 1, 1, 1, 64, 7) == -1          # refused before anything is launched


@pytest.mark.parametrize("nt", P.RANSAC_BLOCKS + P.RANSAC_BLOCKS_ALT)
def test_ransac_block(nt):
    """block_count and the ordered_slot / ordered_commit compaction at the block size of the three solver kernels (256) and of their
    documented 128- and 64-thread builds, against numpy: n = 0, 1, 63, 64, 65, the block size +- 1 and several multiples; all-false,
    all-true and random predicates"""
    rng = np.random.default_rng(0xB10C + nt)
    sizes = sorted({0, 1, 63, 64, 65, nt - 1, nt, nt + 1, 2 * nt, 3 * nt, 5 * nt + 17, 2000})
    for n in sizes:
        for kind in ("none", "all", "random", "sparse"):
            flags = {"none": np.zeros(n, np.int32), "all": np.ones(n, np.int32), "random": rng.integers(0, 2, n).astype(np.int32),
                     "sparse": (rng.uniform(size=n) < 0.05).astype(np.int32)}[kind]
            cnt, running, kept = P.ransac_call(nt, flags)
            want = np.flatnonzero(flags)
            assert cnt == len(want) and running == len(want), (nt, n, kind, cnt, running)
            slots = np.cumsum(flags) - flags                                     # the slot of entry i: the kept entries before it
            assert (kept[:len(want)] == want).all() and (slots[want] == np.arange(len(want))).all(), (nt, n, kind)
            assert (kept[len(want):] == -1).all()
