"""The size tiers of the dense solvers and the Schur plan, read from the product's own formulas through the host-only entry points of
tests/native/libdense_probe.so (no GPU), and the numpy reference of tests/test_dense_solvers_gpu.py held to the bound that file asks of the
kernels.  A moved limit or a changed LDS formula fails here first; tests/test_optimizer_tiers_gpu.py then says which sizes must follow."""
import numpy as np
import pytest

import dense_probe as dp

LDS_SIZES = range(1, 164)                                     # every n ldlt_solve takes
GLOBAL_SIZES = (165, 168, 175, 176, 177, 192, 208, 255, 256, 257, 375, 525, 528, 540)


def test_byte_limits_and_lds_formulas():
    s = dp.sizes(162)
    assert (s["LDS_SOLVER_LIMIT"], s["GLOBAL_SOLVER_LIMIT"], s["PERSISTENT_HS_LIMIT"]) == (156 * 1024, 150 * 1024, 136 * 1024)
    for n in (1, 15, 16, 17, 64, 65, 162, 163, 528):          # dense_ldlt.h: lds_doubles / global_lds_doubles / global_panel_doubles
        prow = (n + 1 + 15) // 16 * 16
        s = dp.sizes(n)
        assert s["lds_doubles"] == (n + 1) * (n + 2) // 2 + 2 * prow * 17 + 16 * 17 + 16 + max(n, 64)
        assert s["global_lds_doubles"] == 16 * 17 + n and s["global_panel_doubles"] == 2 * (n + 16) * 17
    assert 8 * dp.sizes(162)["lds_doubles"] == 158400 and 8 * dp.sizes(168)["lds_doubles"] == 166440


def test_tier_edges_of_the_bundle_adjusters():
    # the LDS-resident solver ends at n = 163: LocalBundleAdjustment (P = 6 nFree) 27 | 28, LocalInertialBA (P = 15 nOpt) 10 | 11
    assert [n for n in range(1, 200) if dp.fits_lds_solver(n)] == list(range(1, 164))
    assert dp.fits_lds_solver(6 * 27) and not dp.fits_lds_solver(6 * 28)
    assert dp.fits_lds_solver(15 * 10) and not dp.fits_lds_solver(15 * 11)
    # k_local_ba (mode=1) keeps Hs | x in LDS up to P = 131: 21 | 22 free keyframes
    assert [P for P in range(1, 200) if dp.persistent_hs_in_lds(P)] == list(range(1, 132))
    assert dp.persistent_hs_in_lds(6 * 21) and not dp.persistent_hs_in_lds(6 * 22)
    # the global-memory solver keeps its panel copies in LDS up to n = 525
    assert [n for n in range(500, 560) if dp.panel_in_lds(n)] == list(range(500, 526))
    assert dp.panel_in_lds(525) and not dp.panel_in_lds(528)
    # even without the panel copies the solver's own LDS (dblk | y) stays far below its limit at every window the tests run
    assert 8 * dp.sizes(900)["global_lds_doubles"] <= dp.sizes(900)["GLOBAL_SOLVER_LIMIT"]


def test_schur_plan_column_blocks_cross_at_the_listed_windows():
    # ncols = 6 n + 1 (matrix columns + the right-hand side) crosses a multiple of 32 between these window sizes
    for lo, hi in ((5, 6), (10, 11), (15, 16), (21, 22)):
        a, b = dp.schur_plan(6 * lo + 1, 3000), dp.schur_plan(6 * hi + 1, 3000)
        assert b["Mp"] == a["Mp"] + 32 and a["Mp"] == (6 * lo + 1 + 31) // 32 * 32, (lo, hi, a, b)
    for nc in (32, 64):                                       # the right-hand side as the LAST column of a block
        assert dp.schur_plan(nc, 100)["Mp"] == nc and dp.schur_plan(nc + 1, 100)["Mp"] == nc + 32


def test_schur_plan_invariants_on_a_grid():
    """k_schur_mfma reads one pipeline group past the last split (wElems covers it), every split is whole groups, and the splits cover K."""
    for ncols in list(range(2, 70)) + list(range(70, 401, 7)) + [400]:
        for K in list(range(1, 200)) + list(range(200, 12001, 97)) + [12000]:
            p = dp.schur_plan(ncols, K)
            assert p["SB"] == 32 and p["Mp"] % 32 == 0 and 0 <= p["Mp"] - ncols < 32
            assert p["nb"] == p["Mp"] // 32 and p["nblk"] == p["nb"] * (p["nb"] + 1) // 2
            assert p["ksteps"] == (K + 3) // 4 and p["nsplit"] >= 1
            assert p["stepsPerSplit"] % p["SU"] == 0 and p["stepsPerSplit"] > 0
            assert p["nsplit"] * p["stepsPerSplit"] >= p["ksteps"] > (p["nsplit"] - 1) * p["stepsPerSplit"]
            assert p["Kp"] == 4 * p["nsplit"] * p["stepsPerSplit"] >= K
            assert p["wElems"] >= (p["Kp"] + 4 * p["SU"]) * p["Mp"]
            assert p["partElems"] == p["nsplit"] * p["nblk"] * 1024


@pytest.mark.parametrize("sizes", [LDS_SIZES, GLOBAL_SIZES], ids=["lds", "global"])
def test_numpy_reference_meets_the_bound_asked_of_the_kernels(sizes):
    """The bound of tests/test_dense_solvers_gpu.py is not too tight: a plain unblocked column LDL^T in float64 meets it at every size,
    with the strict upper triangle valid or NaN."""
    worst = 0.0
    for n in sizes:
        H, b, xs, bound = dp.spd_problem(n)
        Hn = H.copy(); Hn[np.triu_indices(n, 1)] = np.nan
        for M in (H, Hn):
            err = np.abs(dp.ldlt_numpy(M, b) - xs).max()
            assert err <= bound, (n, err, bound)
            worst = max(worst, err / bound)
    print(f"largest error / bound of the numpy reference: {worst:.3g}")


def test_numpy_reference_meets_the_bound_on_the_pivot_problems():
    for n in (41, 96):
        for j in (0, 7, 15, 16, 17, 40, n - 1):
            H, b, xs, bound = dp.pivot_problem(n, j, -4)
            assert np.linalg.eigvalsh(H).min() == pytest.approx(-4.0)            # indefinite, the pivot at j is exactly -4
            err = np.abs(dp.ldlt_numpy(H, b) - xs).max()
            assert err <= bound, (n, j, err, bound)


def test_one_wrong_element_of_L_is_far_outside_the_bound():
    """What the bound detects: ONE entry of L off by a part in 2^20 (far less than a dropped or doubled update of that element) moves x by
    orders of magnitude more than the bound allows, wherever the entry sits."""
    for n in (41, 96, 163, 257):
        H, b, xs, bound = dp.spd_problem(n)
        for r, c in ((1, 0), (n - 1, 0), (n - 1, n - 2), (n // 2, n // 3), (min(n - 1, 17), 15), (min(n - 1, 33), 16)):
            err = np.abs(dp.ldlt_numpy(H, b, corrupt=(r, c, 1 + 2.0 ** -20)) - xs).max()
            assert err > 1e3 * bound, (n, r, c, err, bound)
