"""LocalBundleAdjustment and LocalInertialBA through the C ABI on BOTH sides of every size at which their dense code changes shape, with
the assertions of test_local_ba_matches_oracle / test_local_inertial_ba on graphs small enough for a case to take a second or two:
  * ldlt_solve -> ldlt_solve_global          8 lds_doubles(P) > LDS_SOLVER_LIMIT: LocalBA (P = 6 nFree, grid mode) 27 | 28, inertial (P = 15 nOpt) 10 | 11
  * k_local_ba: Hs in LDS -> in global memory  8 P (P + 1) > PERSISTENT_HS_LIMIT: LocalBA, mode=1, 21 | 22
  * inside ldlt_solve: one partial block (P < 16), a full last block (P % 16 == 0) vs a short one, P across 64 and 128
  * the Schur plan's column blocks: 6 n + 1 across a multiple of 32 at 5 | 6, 10 | 11, 15 | 16, 21 | 22
Which side a size falls on is computed from the product's own formulas and limits (tests/native/libdense_probe.so: probe_sizes,
probe_schur_plan); test_every_tier_edge_has_a_case_on_both_sides fails if a limit moves and the sizes do not follow.
(The edge of the global solver's panel copies, P 525 | 528, is beyond these small graphs: test_dense_solvers_gpu.py runs it on the
solver itself, test_local_inertial_ba at 30 | 45 keyframes through the optimiser.)"""
import numpy as np
import pytest

import dense_probe as dp
import oracle_lib as O
from morb_slam_amd.synth import imu_calib_diagonals, make_ba_problem, make_inertial_ba_problem

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4

BA_NFREE = (1, 2, 3, 5, 6, 8, 10, 11, 16, 21, 22, 24, 27, 28, 32)
IBA_CASES = tuple((n, False) for n in (1, 2, 3, 5, 6, 9, 10, 11, 12, 16, 17)) + ((10, True), (11, True))


def _both_sides(sizes, pred):
    """the adjacent pair (a, b) of `sizes` between which pred changes, or None"""
    s = sorted(sizes)
    flips = [(a, b) for a, b in zip(s[:-1], s[1:]) if pred(a) != pred(b)]
    return flips[0] if len(flips) == 1 else None


def test_every_tier_edge_has_a_case_on_both_sides():
    ba, iba = BA_NFREE, sorted({n for n, _ in IBA_CASES})
    assert _both_sides(ba, lambda n: dp.fits_lds_solver(6 * n)) == (27, 28)                       # grid mode: LDS solver | global solver
    assert _both_sides(ba, lambda n: dp.persistent_hs_in_lds(6 * n)) == (21, 22)                  # mode=1: Hs in LDS | in global memory
    assert _both_sides(iba, lambda n: dp.fits_lds_solver(15 * n)) == (10, 11)
    assert {large for n, large in IBA_CASES if n in (10, 11)} == {False, True}
    for sizes, P in ((ba, lambda n: 6 * n), (iba, lambda n: 15 * n)):
        lds = [P(n) for n in sizes if dp.fits_lds_solver(P(n))]
        assert any(p < dp.NB for p in lds)                                                        # one partial block, no panel below it
        assert any(p % dp.NB and p > dp.NB for p in lds)                                          # a short, identity-padded last block
        assert any(p <= 64 for p in lds) and any(64 < p <= 128 for p in lds) and any(p > 128 for p in lds)   # load and back-substitution pieces
        assert all(dp.panel_in_lds(P(n)) for n in sizes if not dp.fits_lds_solver(P(n)))          # (the global solver's other tier: see the module docstring)
        # Schur plan (6 n + 1 columns in both optimisers): every column-block count up to the largest window's, so both sides of each step
        mp = [dp.schur_plan(6 * n + 1, 3000)["Mp"] for n in sizes]
        assert sorted(set(mp)) == list(range(32, max(mp) + 1, 32))
    assert any(6 * n % dp.NB == 0 for n in ba if dp.fits_lds_solver(6 * n))                       # a full last block (15 nOpt has none below 240)
    for lo, hi in ((5, 6), (10, 11), (21, 22)):                                                   # steps of the plan with both neighbours among the sizes
        assert lo in ba and hi in ba and dp.schur_plan(6 * hi + 1, 3000)["Mp"] == dp.schur_plan(6 * lo + 1, 3000)["Mp"] + 32


@pytest.mark.parametrize("n_free", BA_NFREE)
def test_local_ba_at_the_tier_edges(n_free):
    from morb_slam_amd import Optimizer
    b = make_ba_problem(n_free=n_free, n_fixed=2, n_points=max(60, 12 * (n_free + 2)), seed=40 + n_free)
    opt = Optimizer()
    want = {lam: O.local_ba(b, lambda100=lam) for lam in (False, True)}
    for inertial, mode in ((False, 0), (True, 0), (False, 1), (True, 1)):   # grid mode and persistent-workgroup mode
        run = lambda: opt.LocalBundleAdjustment(b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"],
                                                inertial=inertial, mode=mode)
        kf, mp, erase, stats = run()
        its, kfe, mpe, ee, se = want[inertial]
        tag = (n_free, inertial, mode)
        assert int(stats[0]) == int(se[0]) and int(stats[1]) == int(se[1]), (tag, stats, se)
        assert np.abs(kf - kfe).max() <= POSE_TOL, tag
        assert np.abs(mp - mpe).max() <= 1e-4 * max(1.0, np.abs(mpe).max()), tag
        np.testing.assert_array_equal(erase, ee)
        kf2, mp2, erase2, stats2 = run()                                    # fixed summation orders, no atomics: bit-identical
        assert np.asarray(kf2).tobytes() == np.asarray(kf).tobytes() and np.asarray(mp2).tobytes() == np.asarray(mp).tobytes(), tag
        assert np.asarray(erase2).tobytes() == np.asarray(erase).tobytes() and np.asarray(stats2).tolist() == np.asarray(stats).tolist(), tag
    opt.close()


@pytest.mark.parametrize("n_opt,large", IBA_CASES)
def test_local_inertial_ba_at_the_tier_edges(n_opt, large):
    from morb_slam_amd import Optimizer
    nga, walk = imu_calib_diagonals()
    p = make_inertial_ba_problem(n_opt=n_opt, seed=60 + n_opt, n_points=400)
    pre = np.stack([O.imu_preintegrate(p["bias"], nga, walk, p["acc"][a:b], p["gyro"][a:b], p["dt"][a:b])
                    for a, b in zip(p["imuStart"][:-1], p["imuStart"][1:])])
    r, kf_o, mp_o, er_o, st_o = O.local_inertial_ba(p, pre, bLarge=large)
    opt = Optimizer(0)
    run = lambda: opt.LocalInertialBA(p["kfState"], p["kfKind"], p["mpPos"], p["mpClose"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"],
                                      p["iKF1"], p["iKF2"], pre, p["iRobust"], p["iInfoScale"], p["cam"], p["Tbc12"], bLarge=large)
    kf, mp, er, st = run()
    assert int(st[2]) == r == 1
    assert (int(st[0]), int(st[1])) == (int(st_o[0]), int(st_o[1])), (st, st_o)      # same LM path
    optk = p["kfKind"] == 0
    assert np.allclose(kf[optk], kf_o[optk], rtol=0, atol=1e-4), np.abs(kf[optk] - kf_o[optk]).max()
    assert np.array_equal(kf[~optk], p["kfState"][~optk])                            # fixed keyframes untouched
    d = np.abs(mp - mp_o).max(1) / np.maximum(1.0, np.linalg.norm(mp_o, axis=1))
    assert d.max() < 1e-4, (np.quantile(d, 0.99), d.max())
    np.testing.assert_array_equal(er, er_o)
    kf2, mp2, er2, st2 = run()
    assert kf2.tobytes() == kf.tobytes() and mp2.tobytes() == mp.tobytes() and er2.tobytes() == er.tobytes()
    opt.close()
