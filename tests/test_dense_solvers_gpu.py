"""The dense FP64 kernels under the optimisers, each launched ALONE through tests/native/libdense_probe.so with the sizes and limits the
product uses, against answers that are known exactly:
  * morbdense::ldlt_solve / ldlt_solve_global (dense_ldlt.h), both PIVOT_POSITIVE instantiations: integer SPD systems H x* = b whose H, b
    and x* are exact in FP64, held to the forward bound of a backward-stable LDL^T; the pivot rules on block-diagonal matrices;
  * morbschur::k_schur_mfma + schur_sum4 (schur_mfma.h): integer operands whose every partial sum is exact (bit-equal to the int64
    product), and real operands against numpy within the bound any summation order of K terms meets.
The whole-solve tests (test_optimizer_gpu.py, test_inertial_gpu.py) compare poses to 1e-4 after a self-correcting LM run; a wrong tile
corner or a misplaced split can survive that.  It cannot survive these."""
import numpy as np
import pytest

import dense_probe as dp

pytestmark = pytest.mark.gpu

GLOBAL_SIZES = (165, 168, 175, 176, 177, 192, 208, 255, 256, 257, 375, 525, 528, 540)


def _same_bits(a, b):
    return a.view(np.uint64).tolist() == b.view(np.uint64).tolist()


def _untouched(x):
    return _same_bits(x, np.full(len(x), dp.SENTINEL))


def _solve_checked(solve, H, b, xs, bound, tag):
    """Two solves: status 0 first, ok = 1, bit-identical x, within the bound.  Returns error / bound."""
    st, ok, x = solve(H, b)
    assert st == 0, (tag, st)
    assert ok == 1, tag
    st2, ok2, x2 = solve(H, b)
    assert st2 == 0 and ok2 == 1 and _same_bits(x, x2), tag
    err = np.abs(x - xs).max()
    print(f"{tag}: error {err:.3e} bound {bound:.3e} ratio {err / bound:.3g}")
    assert err <= bound, (tag, err, bound)
    return err / bound


@pytest.mark.parametrize("pivot_positive", [False, True])
def test_ldlt_lds_every_size(pivot_positive):
    """ldlt_solve at EVERY n it takes (1 .. 163): one partial block (n < 16), full and short, identity-padded last blocks, the 64 and 128
    crossings of the load pieces and of the back substitution, up to the last n whose triangle fits LDS.  max |x - x*| <= 8 n u k2(H) max |x*|
    — the plain numpy LDL^T of dense_probe.py meets it with a largest error / bound of 0.018 (test_dense_tiers_cpu.py) — and a wrong or
    missing update of ONE element moves x by many orders of magnitude more (test_dense_tiers_cpu.py: an entry of L off by 2^-20 is
    > 1000 bounds out).  Second family: the strict upper triangle is NaN; the contract says only the lower triangle is read.
    Largest error / bound measured on an MI355X: 0.0101 (n = 4; both instantiations, both families)."""
    nmax = max(n for n in range(1, 193) if dp.fits_lds_solver(n))
    assert nmax == 163
    assert dp.lib().probe_ldlt_lds(int(pivot_positive), 1, 1, 1, nmax + 1, 1) == -2      # refused before anything is launched
    worst = 0.0
    for n in range(1, nmax + 1):
        H, b, xs, bound = dp.spd_problem(n)
        assert np.abs(dp.ldlt_numpy(H, b) - xs).max() <= bound                            # the reference meets the same bound
        Hn = H.copy(); Hn[np.triu_indices(n, 1)] = np.nan
        for fam, M in (("full", H), ("lower", Hn)):
            worst = max(worst, _solve_checked(lambda A, r: dp.solve_lds(pivot_positive, A, r), M, b, xs, bound, f"lds pp={pivot_positive} n={n} {fam}"))
    print(f"largest error / bound: {worst:.3g}")


@pytest.mark.parametrize("pivot_positive", [False, True])
@pytest.mark.parametrize("n", GLOBAL_SIZES)
def test_ldlt_global(n, pivot_positive):
    """ldlt_solve_global just beyond the LDS solver's range, across 176 / 192 / 256 (whole 16-column panels and short last ones), at the
    inertial window of 25 keyframes (375) and on both sides of the size at which its panel copies leave LDS (525 | 528), with the
    placement the product chooses; up to 525 also with the copies forced into global scratch, a legal placement.  Same bound as above.
    Largest error / bound measured on an MI355X: 0.00076 (both instantiations, both placements).
    (No NaN upper triangle here: this solver reads both halves of the diagonal blocks' storage — the upper half through the transposed
    index, i.e. again the lower triangle's values — and its contract is a symmetric matrix.)"""
    assert not dp.fits_lds_solver(n)
    H, b, xs, bound = dp.spd_problem(n)
    assert np.abs(dp.ldlt_numpy(H, b) - xs).max() <= bound
    placements = [dp.panel_in_lds(n)] + ([False] if dp.panel_in_lds(n) else [])
    assert placements[0] == (n <= 525)
    got = []
    for in_lds in placements:
        tag = f"global pp={pivot_positive} n={n} panel_in_lds={int(in_lds)}"
        _solve_checked(lambda A, r: dp.solve_global(pivot_positive, A, r, in_lds), H, b, xs, bound, tag)
        got.append(dp.solve_global(pivot_positive, H, b, in_lds)[2])
    if len(got) == 2:
        assert _same_bits(got[0], got[1])               # where the panel copies live changes no rounding
    if n == 528:                                        # the panel copies no longer fit: the probe refuses what the product never asks for
        assert dp.solve_global(pivot_positive, H, b, True)[0] == -2


@pytest.mark.parametrize("solver", ["lds", "global"])
@pytest.mark.parametrize("n", [41, 96])
def test_pivot_rules(n, solver):
    """H = diag(S1, d, S2) with a 1 x 1 block d at column j: the couplings are exact zeros, so every update of d is exactly zero and the
    pivot at j IS d.  j: the first column, inside / the last of the first block, the first and second of a look-ahead block, a later block,
    the last column (n = 41: in a short last block; n = 96: in a full one).  d = 0 and d = NaN: both instantiations return ok = 0 and leave x
    bit-for-bit untouched.  d = -4: PIVOT_POSITIVE refuses (x untouched), the other rule solves — within the bound with k2 of the
    indefinite matrix.  Handled return paths, not faults: the launch status is 0 throughout."""
    def run(pp, H, b):
        return dp.solve_lds(pp, H, b) if solver == "lds" else dp.solve_global(pp, H, b, True)
    for j in (0, 7, 15, 16, 17, 40, n - 1):
        for d in (0, None):
            H, b, _, _ = dp.pivot_problem(n, j, d)
            for pp in (False, True):
                st, ok, x = run(pp, H, b)
                assert st == 0, (n, j, d, pp, st)
                assert ok == 0 and _untouched(x), (n, j, d, pp, ok)
        H, b, xs, bound = dp.pivot_problem(n, j, -4)
        st, ok, x = run(True, H, b)
        assert st == 0, (n, j, st)
        assert ok == 0 and _untouched(x), (n, j, ok)
        _solve_checked(lambda A, r: run(False, A, r), H, b, xs, bound, f"{solver} n={n} pivot -4 at {j}")


# ---- Schur product -------------------------------------------------------------------------------------------------------------------------
SCHUR_NCOLS = (7, 31, 32, 33, 37, 61, 64, 65, 97, 127, 163, 169, 193)     # 6 n + 1 of real windows, and the multiples of 32 with their neighbours
SCHUR_K = (5, 127, 190, 250, 320, 2111, 2113, 4500)


def _triu_equal_bits(C, R):
    iu = np.triu_indices(C.shape[0])
    return _same_bits(np.ascontiguousarray(C[iu]), np.ascontiguousarray(R[iu]))


def test_schur_shapes_cover_every_path_of_the_plan():
    """The plans of SCHUR_NCOLS x SCHUR_K, read from the product's make_plan: nsplit 1 .. 5 (schur_sum4's quarters of 1 or 2 splits, some
    EMPTY), nsplit >= 33 (a quarter of >= 8 splits: the unrolled-by-8 loop and its tail both run), K % 4 != 0 (a partial last k-step),
    K one below and one above a multiple of 4 stepsPerSplit (a last split that is full but for one row / holds a single row), one to
    seven column blocks."""
    plans = [dict(dp.schur_plan(nc, K), K=K, ncols=nc) for nc in SCHUR_NCOLS for K in SCHUR_K]
    ns = {p["nsplit"] for p in plans}
    assert {1, 2, 3, 4, 5} <= ns and max(ns) >= 33
    tails = {((p["nsplit"] + 3) // 4) % 8 for p in plans if (p["nsplit"] + 3) // 4 >= 8}
    assert any(t != 0 for t in tails)                                            # the loop by 8 AND its tail
    assert any(p["K"] % 4 != 0 for p in plans) and any(p["K"] % 4 == 0 for p in plans)
    assert any(p["K"] % (4 * p["stepsPerSplit"]) == 4 * p["stepsPerSplit"] - 1 for p in plans)
    assert any(p["K"] % (4 * p["stepsPerSplit"]) == 1 and p["nsplit"] > 1 for p in plans)
    assert {p["nb"] for p in plans} == {1, 2, 3, 4, 6, 7}
    assert any(p["ncols"] == p["Mp"] for p in plans)                            # the right-hand side is the last column of a block
    assert all(p["K"] <= 4500 for p in plans)


@pytest.mark.parametrize("ncols", SCHUR_NCOLS)
def test_schur_exact_integers(ncols):
    """W, WD: integers in [-4, 4], ~75 % zeros as on real graphs.  Every product and every partial sum is an exactly representable integer
    (|sum| <= 16 K < 2^53), so whatever the order C must be BIT-equal to the int64 product on i <= j: a mis-indexed lane, a dropped split
    or a non-zero spare group shows.  Zero tolerance."""
    for K in SCHUR_K:
        rng = np.random.default_rng(0x5C + 100000 * ncols + K)
        W, WD = (rng.integers(-4, 5, (K, ncols)) * (rng.random((K, ncols)) < 0.25) for _ in range(2))
        ref = (WD.astype(np.int64).T @ W.astype(np.int64)).astype(np.float64)
        st, Cm, p = dp.schur(W, WD)
        assert st == 0, (ncols, K, st)
        assert not np.isnan(Cm[np.triu_indices(ncols)]).any(), (ncols, K, p)
        assert _triu_equal_bits(Cm, ref), (ncols, K, p, np.argwhere(np.triu(Cm != ref)))


@pytest.mark.parametrize("ncols", SCHUR_NCOLS)
def test_schur_real_values(ncols):
    """Magnitudes 2^-20 .. 2^20, mixed signs, ~75 % zeros: |C - C64| <= 2 (K + 4) u (|WD|^T |W|) with C64 numpy's float64 product — each
    side carries at most gamma_K of that sum whatever its summation order (the kernel adds nsplit partials and four quarters on top of
    the k-steps: fewer than K + 4 additions per element).  A second run is bit-identical (fixed split and quarter order, no atomics)."""
    for K in SCHUR_K:
        rng = np.random.default_rng(0x5EA1 + 100000 * ncols + K)
        W, WD = (np.ldexp(rng.uniform(0.5, 1.0, (K, ncols)), rng.integers(-20, 21, (K, ncols))) * rng.choice([-1.0, 1.0], (K, ncols))
                 * (rng.random((K, ncols)) < 0.25) for _ in range(2))
        ref = WD.T @ W
        tol = 2 * (K + 4) * dp.U * (np.abs(WD).T @ np.abs(W))
        st, Cm, p = dp.schur(W, WD)
        assert st == 0, (ncols, K, st)
        iu = np.triu_indices(ncols)
        assert not np.isnan(Cm[iu]).any(), (ncols, K, p)
        assert (np.abs(Cm - ref)[iu] <= tol[iu]).all(), (ncols, K, p, (np.abs(Cm - ref)[iu] / np.maximum(tol[iu], 1e-300)).max())
        st2, C2, _ = dp.schur(W, WD)
        assert st2 == 0 and _triu_equal_bits(Cm, C2), (ncols, K)
