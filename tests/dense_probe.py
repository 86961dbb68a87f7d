"""Helpers of the dense-solver tests: the ctypes face of tests/native/libdense_probe.so (tests/native/dense_probe.hip — the LDL^T solvers of
dense_ldlt.h and the MFMA Schur product of schur_mfma.h behind thin entry points), problems whose exact answer is known, a plain numpy
LDL^T, and the size tiers of the two bundle adjusters worked out from the formulas the product uses."""
import ctypes as C
import functools
import os

import numpy as np

U = 2.0 ** -53                      # unit roundoff of FP64
NB = 16                             # panel width of both solvers (dense_ldlt.h: NB)
_lib = None


def lib():
    """The probe library.  Loading it needs no GPU; torch first, so that it binds to the HIP runtime torch brought (morb_slam_amd/capi.py)."""
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        from morb_slam_amd import build
        L = C.CDLL(os.environ.get("MORB_DENSE_PROBE_LIB") or build.build_dense_probe())   # (a scratch build with one thing broken points this at itself)
        vp, i32, pll = C.c_void_p, C.c_int, C.POINTER(C.c_longlong)
        L.probe_sizes.restype, L.probe_sizes.argtypes = i32, [i32, pll]
        L.probe_schur_plan.restype, L.probe_schur_plan.argtypes = i32, [i32, i32, pll]
        L.probe_ldlt_lds.restype, L.probe_ldlt_lds.argtypes = i32, [i32, vp, vp, vp, i32, vp]
        L.probe_ldlt_global.restype, L.probe_ldlt_global.argtypes = i32, [i32, vp, vp, vp, i32, i32, vp, vp]
        L.probe_schur.restype, L.probe_schur.argtypes = i32, [i32, i32, vp, vp, vp, vp, vp, vp, pll]
        _lib = L
    return _lib


# ---- sizes and tiers ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sizes(n):
    """dict of lds_doubles / global_lds_doubles / global_panel_doubles at n and the three byte limits (dense_ldlt.h)."""
    out = (C.c_longlong * 6)()
    assert lib().probe_sizes(n, out) == 0
    return dict(zip(("lds_doubles", "global_lds_doubles", "global_panel_doubles", "LDS_SOLVER_LIMIT", "GLOBAL_SOLVER_LIMIT",
                     "PERSISTENT_HS_LIMIT"), [int(v) for v in out]))


def fits_lds_solver(n):
    """ldlt_solve is the solver of an n x n system (local_ba.hip: denseLds, inertial_ba.hip: denseLds)."""
    s = sizes(n)
    return 8 * s["lds_doubles"] <= s["LDS_SOLVER_LIMIT"]


def panel_in_lds(n):
    """ldlt_solve_global keeps its panel copies in LDS (local_ba.hip / inertial_ba.hip: panelInLds)."""
    s = sizes(n)
    return 8 * (s["global_lds_doubles"] + s["global_panel_doubles"]) <= s["GLOBAL_SOLVER_LIMIT"]


def persistent_hs_in_lds(P):
    """k_local_ba (LocalBundleAdjustment, mode=1) keeps Hs | x in LDS (local_ba.hip: useLds)."""
    return 8 * P * (P + 1) <= sizes(max(P, 1))["PERSISTENT_HS_LIMIT"] and P <= 192


PLAN_FIELDS = ("Mp", "nb", "nblk", "Kp", "ksteps", "nsplit", "stepsPerSplit", "wElems", "partElems", "SB", "SU")


@functools.lru_cache(maxsize=None)
def schur_plan(ncols, K):
    out = (C.c_longlong * 11)()
    assert lib().probe_schur_plan(ncols, K, out) == 0
    return dict(zip(PLAN_FIELDS, [int(v) for v in out]))


# ---- problems with an exactly known answer ---------------------------------------------------------------------------------------------
def spd_integer(n, rng):
    """H = G G^T + n I with G integer in [-3, 3]: SPD, every entry an exact FP64 integer."""
    G = rng.integers(-3, 4, (n, n)).astype(np.int64)
    return G @ G.T + n * np.eye(n, dtype=np.int64)


def with_solution(Hi, rng):
    """(H, b, x*) in FP64 for the int64 matrix Hi: x* integer in [-8, 8], b = H x* computed in int64 — all exact, x* IS the solution."""
    xs = rng.integers(-8, 9, Hi.shape[0]).astype(np.int64)
    b = Hi @ xs
    assert np.abs(b).max() < 2 ** 53 and np.abs(Hi).max() < 2 ** 53
    return Hi.astype(np.float64), b.astype(np.float64), xs.astype(np.float64)


@functools.lru_cache(maxsize=None)
def spd_problem(n, seed=0):
    rng = np.random.default_rng(0xD5E + 1000 * seed + n)
    H, b, xs = with_solution(spd_integer(n, rng), rng)
    return H, b, xs, forward_bound(H, xs)


@functools.lru_cache(maxsize=None)
def pivot_problem(n, j, d):
    """H = diag(S1, d, S2): a 1 x 1 block d at column j with zero couplings, so every update of it is exactly zero and pivot j IS d.
    d: an integer, or None for NaN.  Returns (H, b, x*, bound) — x* and the bound are meaningful for a non-zero, finite d only."""
    rng = np.random.default_rng(0xB10C + 1000 * n + j)
    Hi = np.zeros((n, n), np.int64)
    if j > 0:
        Hi[:j, :j] = spd_integer(j, rng)
    if j < n - 1:
        Hi[j + 1:, j + 1:] = spd_integer(n - 1 - j, rng)
    Hi[j, j] = 1 if d is None else d
    H, b, xs = with_solution(Hi, rng)
    bound = forward_bound(H, xs) if d not in (None, 0) else None
    if d is None:
        H[j, j] = np.nan
    return H, b, xs, bound


def forward_bound(H, xs):
    """max |x - x*| a backward-stable LDL^T may leave: 8 n u k2(H) max |x*| (the 8 covers the <= 1 ulp reciprocal of the diagonal block)."""
    n = H.shape[0]
    return 8 * n * U * np.linalg.cond(H, 2) * np.abs(xs).max()


def ldlt_numpy(H, b, corrupt=None):
    """Plain unblocked column LDL^T in float64 (no pivoting) and the two substitutions.  corrupt = (r, c, factor): L[r][c] is multiplied by
    factor after the factorisation — what a wrong update of one element looks like to the solve."""
    n = H.shape[0]
    A = np.tril(H)                                                              # (only the lower triangle is read, as by ldlt_solve)
    L = np.eye(n)
    D = np.zeros(n)
    for j in range(n):
        D[j] = A[j, j]
        L[j + 1:, j] = A[j + 1:, j] / D[j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], A[j + 1:, j])
    if corrupt is not None:
        L[corrupt[0], corrupt[1]] *= corrupt[2]
    y = b.copy()
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y /= D
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    return y


# ---- launches --------------------------------------------------------------------------------------------------------------------------
SENTINEL = np.array([0x7FF8DEADBEEF1234], np.uint64).view(np.float64)[0]     # a NaN with a payload: "x untouched" is a comparison of bits


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def solve_lds(pivot_positive, H, b):
    """ldlt_solve<pivot_positive> on the GPU: (status, ok, x); x was prefilled with SENTINEL."""
    import torch
    n = H.shape[0]
    dH, db = _dev(H), _dev(b)
    dx = _dev(np.full(n, SENTINEL))
    ok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = lib().probe_ldlt_lds(int(pivot_positive), dH.data_ptr(), db.data_ptr(), dx.data_ptr(), n, ok.data_ptr())
    if st != 0:
        return st, None, None
    return st, int(ok.item()), dx.cpu().numpy()


def solve_global(pivot_positive, H, b, in_lds):
    """ldlt_solve_global<pivot_positive> on the GPU, panel copies in LDS or in global scratch: (status, ok, x)."""
    import torch
    n = H.shape[0]
    dA, db = _dev(H.copy()), _dev(b)                                            # (A is overwritten by the factors: a copy)
    dx = _dev(np.full(n, SENTINEL))
    pnl = torch.zeros((sizes(n)["global_panel_doubles"],), dtype=torch.float64, device="cuda")
    ok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = lib().probe_ldlt_global(int(pivot_positive), dA.data_ptr(), db.data_ptr(), dx.data_ptr(), n, int(in_lds), pnl.data_ptr(), ok.data_ptr())
    if st != 0:
        return st, None, None
    return st, int(ok.item()), dx.cpu().numpy()


def schur(W, WD):
    """C = WD^T W on the GPU (k_schur_mfma + schur_sum4) for [K][ncols] operands: (status, C, plan); C is NaN below the diagonal."""
    import torch
    K, ncols = W.shape
    p = schur_plan(ncols, K)
    ops = []
    for a in (W, WD):
        t = torch.zeros((p["wElems"],), dtype=torch.float64, device="cuda")
        t[:p["Kp"] * p["Mp"]].view(p["Kp"], p["Mp"])[:K, :ncols] = _dev(a.astype(np.float64))
        ops.append(t)
    part = torch.full((p["partElems"],), float("nan"), dtype=torch.float64, device="cuda")
    blocks = torch.zeros((2 * p["nblk"],), dtype=torch.int32, device="cuda")
    blkIndex = torch.zeros((p["nb"] * p["nb"],), dtype=torch.int32, device="cuda")
    Cm = torch.full((ncols, ncols), float("nan"), dtype=torch.float64, device="cuda")
    out = (C.c_longlong * 11)()
    torch.cuda.synchronize()
    st = lib().probe_schur(ncols, K, ops[0].data_ptr(), ops[1].data_ptr(), part.data_ptr(), blocks.data_ptr(), blkIndex.data_ptr(),
                           Cm.data_ptr(), out)
    if st != 0:
        return st, None, None
    assert dict(zip(PLAN_FIELDS, [int(v) for v in out])) == p
    return st, Cm.cpu().numpy(), p
