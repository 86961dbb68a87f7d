"""Sim3Solver on the GPU (morb_sim3_solver_batch) against the CPU oracle (tests/native/sim3_solver_oracle.cc), exactly: per-iteration
inlier counts, converged iteration, nInliers, the mask, iterations done, N, the budget and the bits of T12 / R / t / s.  One seeded
corpus: Pinhole and KannalaBrandt8 on either side, free and fixed scale, 0 / 30 / 60 / 90 % outliers, N = 0, N < minInliers,
N == minInliers (budget 1), no convergence within the budget, degenerate triples and N beyond the LDS.  Chunked iterate(20) ==
one call == the oracle's chunks, batch == alone, rerun == first run."""
import numpy as np
import pytest
import torch

import sim3_solver_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import libc_rand, make_sim3_solver_problem, pack_sim3_solver_problems

pytestmark = pytest.mark.gpu

CLEAN = dict(outlier_frac=0.0, noise_px=0.0, dup_frac=0.0, bad_frac=0.0, no_mp1_frac=0.0, neg_idx_frac=0.0, unmatched_frac=0.0)


def _specs():
    s = []
    cams = [("pinhole", "pinhole"), ("kb8", "pinhole"), ("pinhole", "kb8"), ("kb8", "kb8")]
    for k, (c1, c2) in enumerate(cams):
        for j, of in enumerate((0.0, 0.3, 0.6, 0.9)):
            s.append(dict(n=300 + 37 * j + 11 * k, cam1=c1, cam2=c2, fix_scale=(j + k) % 2 == 1, outlier_frac=of))
    s += [dict(n=0),                                                              # N = 0
          dict(n=40, unmatched_frac=1.0),                                          # no match at all: N = 0
          dict(n=12, **CLEAN),                                                     # N < minInliers (20)
          dict(n=20, **CLEAN),                                                     # N == minInliers: budget 1
          dict(n=20, **dict(CLEAN, outlier_frac=0.5)),                             # budget 1, no convergence
          dict(n=300, min_inliers=280, outlier_frac=0.2),                          # cannot converge: the whole budget
          dict(n=400, outlier_frac=0.6, max_iterations=7),                         # a small maxIterations
          dict(n=60, collinear=True, **dict(CLEAN, noise_px=0.0)),                 # every triple collinear
          dict(n=80, dup_frac=0.9, outlier_frac=0.3),                              # mostly repeated points
          dict(n=30, identical=True, **CLEAN),                                     # every triple repeats one point: NaN hypotheses
          dict(n=5, dup_frac=1.0, min_inliers=3, **{k: v for k, v in CLEAN.items() if k != "dup_frac"}),
          dict(n=3000, outlier_frac=0.5, min_inliers=30),                          # N beyond the LDS path
          dict(n=2500, cam1="kb8", cam2="kb8", outlier_frac=0.7, fix_scale=True, min_inliers=30),
          dict(n=1030, outlier_frac=0.0, noise_px=0.5, unmatched_frac=0.0, bad_frac=0.0, no_mp1_frac=0.0, neg_idx_frac=0.0, dup_frac=0.0),
          dict(n=500, bad_frac=0.3, no_mp1_frac=0.2, neg_idx_frac=0.3, outlier_frac=0.3, probability=0.999, min_inliers=15)]
    return s


def _problems(specs, seed0=0):
    probs, rands = [], []
    for k, sp in enumerate(specs):
        sp = dict(sp)
        sp.setdefault("min_inliers", 20)
        probs.append(make_sim3_solver_problem(seed=seed0 + k, **sp))
        rands.append(libc_rand(1000 + seed0 + k, 3 * probs[-1]["max_iterations"]))
    return probs, rands


def _run(opt, probs, rands, chunk=None, cap=None):
    t = pack_sim3_solver_problems(probs, "cuda:0", rand=rands, cap=cap)
    P = len(probs)
    hyp_cap = max(p["max_iterations"] for p in probs)
    hyp = torch.full((P, hyp_cap), -1, dtype=torch.int32, device="cuda:0")
    mask = None
    if chunk is None:
        st, mask, _ = opt.Sim3Solver(t["params"], t["entry"], t["Xw1"], t["Xw2"], t["sigma2_1"], t["sigma2_2"], t["rand"], t["state"],
                                     hyp_cap, hypInliers=hyp)
        return Optimizer.sim3_solver_state(st), mask.cpu().numpy(), hyp.cpu().numpy(), 1
    calls = 0
    while True:   # LoopClosing: while (!bConverge && !bNoMore) iterate(20, ...), all problems at once until all are done
        st, mask, _ = opt.Sim3Solver(t["params"], t["entry"], t["Xw1"], t["Xw2"], t["sigma2_1"], t["sigma2_2"], t["rand"], t["state"],
                                     chunk, hypInliers=hyp)
        calls += 1
        s = Optimizer.sim3_solver_state(st)
        if ((s["converged"] != 0) | (s["noMore"] != 0)).all():
            return s, mask.cpu().numpy(), hyp.cpu().numpy(), calls


def _bits(a):
    """float32 bits, every NaN as one pattern (degenerate triples give NaN; its sign and payload are not the reference's business)."""
    a = np.array(a, np.float32, ndmin=1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def _check(p, rand, s, mask, hyp, calls=None):
    oc, best = sim3_solver_oracle.run(p, rand, calls=calls, hyp_cap=len(hyp))
    o = oc[-1]
    n = p["n"]
    assert (s["N"], s["budget"]) == (o["N"], o["budget"])
    assert (s["converged"], s["noMore"], s["nInliers"], s["iterations"], s["bestInliers"]) == \
        (o["converged"], o["noMore"], o["nInliers"], o["iterations"], o["bestInliers"])
    assert np.array_equal(hyp, best["hyp"])
    assert s["convergedAt"] == (o["iterations"] - 1 if o["converged"] else -1)
    assert np.array_equal(mask[:n], o["mask"]) and not mask[n:].any()
    if o["iterations"] > 0:
        assert np.array_equal(_bits(s["bestT12"]), _bits(best["bestT12"]))
        assert np.array_equal(_bits(s["bestR"]), _bits(best["bestR"]))
        assert np.array_equal(_bits(s["bestt"]), _bits(best["bestt"]))
        assert np.array_equal(_bits(s["bestScale"]), _bits(best["bestScale"]))
    if calls is None or len(oc) == 1:
        assert np.array_equal(_bits(s["sim3"]), _bits(o["sim3"]))
    return o


@pytest.fixture(scope="module")
def opt():
    o = Optimizer(0)
    yield o
    o.close()


@pytest.fixture(scope="module")
def corpus():
    return _problems(_specs())


def test_sim3_solver_matches_oracle_exactly(opt, corpus):
    probs, rands = corpus
    s, mask, hyp, _ = _run(opt, probs, rands)
    outcomes = []
    for k, p in enumerate(probs):
        o = _check(p, rands[k], s[k], mask[k], hyp[k])
        outcomes.append((o["converged"], o["noMore"], o["N"], o["budget"], o["iterations"]))
    conv = [c for c, *_ in outcomes]
    assert sum(conv) >= 16 and sum(1 for c, nm, *_ in outcomes if nm and not c) >= 4
    assert any(N == 0 for _, _, N, _, _ in outcomes) and any(b == 1 and N == 20 for _, _, N, b, _ in outcomes)
    assert any(N > 1024 for _, _, N, _, _ in outcomes)
    assert any(it > 1 and c for c, _, _, _, it in outcomes)


def test_chunked_iterate_equals_one_call_and_the_oracle(opt, corpus):
    probs, rands = corpus
    cap = max(p["n"] for p in probs)
    one = _run(opt, probs, rands)
    ncalls = []
    for k in range(len(probs)):   # each problem on its own: LoopClosing stops calling a solver once it converged or has no more
        s, mask, hyp, calls = _run(opt, [probs[k]], [rands[k]], chunk=20, cap=cap)
        ncalls.append(calls)
        for f in ("N", "budget", "iterations", "bestInliers", "converged", "noMore", "nInliers", "convergedAt", "bestT12", "bestR", "bestt",
                  "bestScale"):
            assert np.array_equal(_bits(s[0][f]), _bits(one[0][k][f])), (k, f)
        assert np.array_equal(mask[0], one[1][k]) and np.array_equal(hyp[0], one[2][k, :hyp.shape[1]])
        _check(probs[k], rands[k], s[0], mask[0], hyp[0], calls=[20] * calls)
    assert max(ncalls) == 15   # a problem that runs its whole budget of 300 in 15 calls


def test_batch_equals_alone_and_rerun(opt, corpus):
    probs, rands = corpus
    cap = max(p["n"] for p in probs)
    a = _run(opt, probs, rands)
    b = _run(opt, probs, rands)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for k in (0, 5, 13, len(probs) - 4, len(probs) - 1):
        s, mask, hyp, _ = _run(opt, [probs[k]], [rands[k]], cap=cap)
        assert s[0].tobytes() == a[0][k].tobytes()
        assert np.array_equal(mask[0], a[1][k])
        assert np.array_equal(hyp[0, :a[2].shape[1]], a[2][k, :hyp.shape[1]])
