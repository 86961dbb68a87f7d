"""MLPnPsolver on the GPU (morb_mlpnp_solver_batch) against the CPU oracle (tests/native/mlpnp_solver_oracle.cc) on the seeded corpus
of tests/mlpnp_solver_corpus.py.  Exactly: N, the adjusted minInliers, the budget, iterations, bestInliers, ok, noMore, nInliers,
refined, returnedAt, the inlier count of every evaluated iteration, vbInliers and mvbBestInliers, zeros beyond n.  Within 1e-4
absolute (the project's pose gate): Tcw and bestTcw whenever the oracle's best count reaches minInliers.

Calls: iterate's loop condition is an OR, so the first iterate(5) of a solver runs its whole budget unless Refine() returns first;
the "chunks" of Tracking::Relocalization are therefore repeated iterate(5) calls on the same solver, each continuing from the state
the previous one left (a call after the budget is spent runs exactly five iterations more).  The tests compare (a) the first call,
(b) six consecutive iterate(5) calls, call by call, with the oracle driven the same way, (c) one call with nIterations = the budget
with the first iterate(5) call wherever the budget is at least 5, (d) batch against alone and a rerun, byte for byte."""
import numpy as np
import pytest
import torch

import mlpnp_solver_corpus
import mlpnp_solver_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.synth import pack_mlpnp_problems

pytestmark = pytest.mark.gpu

INT_FIELDS = ("N", "minInliers", "budget", "iterations", "bestInliers", "ok", "noMore", "nInliers", "refined", "returnedAt")
POSE_TOL = 1e-4
NCALLS = 6


@pytest.fixture(scope="module")
def opt():
    o = Optimizer(0)
    yield o
    o.close()


@pytest.fixture(scope="module")
def corpus():
    probs, rands = mlpnp_solver_corpus.problems()
    hyp_cap = max(p["max_iterations"] for p in probs) + 5 * NCALLS
    oracle = [mlpnp_solver_oracle.run(p, r, calls=[5] * NCALLS, stop=False, hyp_cap=hyp_cap) for p, r in zip(probs, rands)]
    return probs, rands, oracle, hyp_cap


def _run(opt, probs, rands, hyp_cap, calls, cap=None):
    """Consecutive calls iterate(calls[k]) on every problem of the batch; returns per call (state records, vbInliers, mvbBestInliers,
    the per-iteration counts so far)."""
    t = pack_mlpnp_problems(probs, "cuda:0", rand=rands, cap=cap)
    hyp = torch.full((len(probs), hyp_cap), -1, dtype=torch.int32, device="cuda:0")
    out = []
    for nit in calls:
        st, mask, _ = opt.MLPnPsolver(t["params"], t["entry"], t["uv"], t["sigma2"], t["Xw"], t["rand"], t["state"], t["bestInliers"], nit,
                                      hypInliers=hyp)
        out.append((Optimizer.mlpnp_solver_state(st), mask.cpu().numpy(), t["bestInliers"].cpu().numpy(), hyp.cpu().numpy()))
    return out


def _check_call(k, c, p, s, mask, best, o, dev):
    n = p["n"]
    for f in INT_FIELDS:
        assert int(s[f]) == o[f], (k, c, f, int(s[f]), o[f])
    assert np.array_equal(mask[:n], o["mask"]) and not mask[n:].any(), (k, c)
    assert np.array_equal(best[:n], o["bestMask"]) and not best[n:].any(), (k, c)
    if o["bestInliers"] >= o["minInliers"] and o["N"] >= o["minInliers"]:
        d = max(float(np.abs(s["Tcw"] - o["Tcw"]).max()), float(np.abs(s["bestTcw"] - o["bestTcw"]).max()))
        dev.append(d)
        print(f"problem {k} call {c}: largest |Tcw - oracle| {d:.3e}")
        assert d <= POSE_TOL, (k, c, d)
    else:
        assert np.array_equal(s["Tcw"], np.eye(4, dtype=np.float32).reshape(-1)), (k, c)


def test_mlpnp_solver_matches_oracle_exactly(opt, corpus):
    probs, rands, oracle, hyp_cap = corpus
    got = _run(opt, probs, rands, hyp_cap, [5])[0]
    dev, first = [], []
    for k, p in enumerate(probs):
        calls, summ = oracle[k]
        o = calls[0]
        _check_call(k, 0, p, got[0][k], got[1][k], got[2][k], o, dev)
        it = o["iterations"]
        assert np.array_equal(got[3][k][:it], summ["hyp"][:it]) and (got[3][k][it:] == -1).all(), k
        first.append(o)
    print(f"largest pose deviation on the device: {max(dev):.3e}")
    sp = mlpnp_solver_corpus.specs()
    assert sum(1 for o in first if o["ok"] and o["refined"]) >= 8
    assert sum(1 for o in first if o["ok"] and not o["refined"]) >= 1
    assert sum(1 for o in first if o["noMore"] and not o["ok"]) >= 3
    assert any(s.get("planar") and o["ok"] for s, o in zip(sp, first))
    assert any(o["N"] > mlpnp_solver_corpus.LDS_N and o["ok"] for o in first)
    assert any(o["ok"] and o["returnedAt"] > 0 for o in first)
    assert any(o["N"] == 0 for o in first) and any(o["N"] == o["minInliers"] and o["budget"] == 1 for o in first)
    assert any(0 < o["N"] < o["minInliers"] for o in first) and any(s.get("min_set") == 8 for s in sp)


def test_consecutive_iterate5_calls_equal_the_oracles_and_one_call_with_the_budget(opt, corpus):
    probs, rands, oracle, hyp_cap = corpus
    got = _run(opt, probs, rands, hyp_cap, [5] * NCALLS)
    dev = []
    for c in range(NCALLS):
        for k, p in enumerate(probs):
            calls, summ = oracle[k]
            _check_call(k, c, p, got[c][0][k], got[c][1][k], got[c][2][k], calls[c], dev)
            it = calls[c]["iterations"]
            assert np.array_equal(got[c][3][k][:it], summ["hyp"][:it]), (k, c)
    # a solver that has spent its budget runs exactly five more iterations per call
    assert any(calls[0]["noMore"] and calls[1]["iterations"] == calls[0]["iterations"] + 5 for calls, _ in oracle)
    first = got[0]
    for k, p in enumerate(probs):   # one call with the whole budget: the same call wherever the budget is at least 5
        b = oracle[k][1]["budget"]
        if b < 5 or oracle[k][1]["N"] < oracle[k][1]["minInliers"]:
            continue
        one = _run(opt, [p], [rands[k]], hyp_cap, [b], cap=first[1].shape[1])[0]
        assert one[0][0].tobytes() == first[0][k].tobytes(), k
        assert np.array_equal(one[1][0], first[1][k]) and np.array_equal(one[2][0], first[2][k]) and np.array_equal(one[3][0], first[3][k])


def test_batch_equals_alone_and_rerun(opt, corpus):
    probs, rands, _, hyp_cap = corpus
    a = _run(opt, probs, rands, hyp_cap, [5, 5])
    b = _run(opt, probs, rands, hyp_cap, [5, 5])
    for c in range(2):
        assert a[c][0].tobytes() == b[c][0].tobytes()
        assert all(np.array_equal(a[c][j], b[c][j]) for j in (1, 2, 3))
    cap = a[0][1].shape[1]
    for k in (1, 9, 16, 20, 22, len(probs) - 2):
        one = _run(opt, [probs[k]], [rands[k]], hyp_cap, [5, 5], cap=cap)
        for c in range(2):
            assert one[c][0][0].tobytes() == a[c][0][k].tobytes(), (k, c)
            assert all(np.array_equal(one[c][j][0], a[c][j][k]) for j in (1, 2, 3)), (k, c)
