"""TwoViewReconstruction on the GPU (morb_two_view_reconstruction_batch) against the CPU oracle (tests/native/two_view_oracle.cc) on the
seeded corpus of tests/two_view_corpus.py.  Exactly: ok, N, the model, both best iterations, both best masks and the chosen mask's
count, nGood of every motion hypothesis, the chosen hypothesis, the failure code, vbTriangulated, zeros beyond n, and (as float bit
patterns, NaN being one pattern) the score of every iteration, SH and SF.  Within the project's 1e-4 gate: T21 (absolute) and every point of vP3D (relative
to max(1, |X|)); both sides run one float sequence, so the deviation printed is expected to be 0.  Also: the batch against one
problem at a time and a rerun, byte for byte; a caller's stream; the three argument refusals; and the chain
SearchForInitialization -> TwoViewReconstruction on one stream with no host copy in between."""
import numpy as np
import pytest
import torch

import two_view_corpus
import two_view_oracle
from morb_slam_amd import Optimizer
from morb_slam_amd.capi import ERR_INVALID, lib, ptr
from morb_slam_amd.optimizer import TWO_VIEW_FSTATS, TWO_VIEW_STATS
from morb_slam_amd.synth import libc_rand, make_two_view_problem, pack_two_view_problems

pytestmark = pytest.mark.gpu

GATE = 1e-4
S = {n: k for k, n in enumerate(TWO_VIEW_STATS)}
F = {n: k for k, n in enumerate(TWO_VIEW_FSTATS)}


@pytest.fixture(scope="module")
def opt():
    o = Optimizer(0)
    yield o
    o.close()


@pytest.fixture(scope="module")
def corpus():
    probs, rands = two_view_corpus.problems()
    return probs, rands, [two_view_oracle.run(p, r) for p, r in zip(probs, rands)]


def _groups(probs):
    """Problem indices by maxIterations: the entry takes one value per call."""
    g = {}
    for k, p in enumerate(probs):
        g.setdefault(p["max_iterations"], []).append(k)
    return g


def _run(opt, probs, rands, cap=None, stream=None):
    """One call per maxIterations group; returns per problem a dict of numpy arrays."""
    res = [None] * len(probs)
    for it, idx in _groups(probs).items():
        t = pack_two_view_problems([probs[k] for k in idx], "cuda:0", rand=[rands[k] for k in idx], cap=cap)
        o = opt.TwoViewReconstruction(t["img1"], t["img2"], t["count"], t["kps"], t["matches12"], t["K4"], t["sigma"], t["rand"], it,
                                      masks=True, hypScores=True, stream=stream)
        if stream is not None:
            torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in o.items()}
        for j, k in enumerate(idx):
            res[k] = {key: v[j] for key, v in o.items()}
    return res


def _bits(a):
    """Float bit patterns; every NaN is one pattern (a sample of fewer than four distinct points scores NaN on both sides, and the sign
    and payload of a NaN are not a value: the x86 and the GPU default NaNs differ in the sign bit)."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _check(k, p, g, o, dev):
    n1, N = p["n1"], o["N"]
    assert int(g["ok"]) == o["ok"], k
    for name in TWO_VIEW_STATS:
        assert int(g["stats"][S[name]]) == o[name], (k, name, int(g["stats"][S[name]]), o[name])
    assert np.array_equal(g["inliersH"][:N], o["inliersH"]) and not g["inliersH"][N:].any(), k
    assert np.array_equal(g["inliersF"][:N], o["inliersF"]) and not g["inliersF"][N:].any(), k
    assert np.array_equal(_bits(g["hypScores"]), _bits(o["hyp"])), (k, "scores")
    assert np.array_equal(_bits(g["fstats"][[F["SH"], F["SF"]]]), _bits(o["fstats"][[F["SH"], F["SF"]]])), (k, "SH SF")
    assert np.array_equal(g["triangulated"][:n1], o["triangulated"]) and not g["triangulated"][n1:].any(), k
    assert not g["P3D"][n1:].any(), k
    if not o["ok"]:
        assert not g["T21"].any() and not g["P3D"].any() and not g["triangulated"].any(), k
        return
    dT = float(np.abs(g["T21"] - o["T21"]).max())
    X = o["P3D"]
    dX = float((np.linalg.norm(g["P3D"][:n1] - X, axis=1) / np.maximum(1.0, np.linalg.norm(X, axis=1))).max())
    dRest = float(np.nanmax(np.abs(g["fstats"] - o["fstats"]) / np.maximum(1.0, np.abs(o["fstats"]))))
    dev.append(max(dT, dX))
    print(f"problem {k} ({p['kind']}): |T21 - oracle| {dT:.3e}, vP3D {dX:.3e}, fstats {dRest:.3e}")
    assert dT <= GATE and dX <= GATE and dRest <= GATE, (k, dT, dX, dRest)
    assert np.array_equal(g["P3D"][:n1].any(axis=1), X.any(axis=1)), k


def test_two_view_matches_oracle(opt, corpus):
    probs, rands, oracle = corpus
    got = _run(opt, probs, rands)
    dev = []
    for k, p in enumerate(probs):
        _check(k, p, got[k], oracle[k], dev)
    print(f"largest deviation of T21 / vP3D on the device: {max(dev):.3e}")
    two_view_corpus.assert_composition(probs, oracle)


def test_batch_equals_alone_and_rerun(opt, corpus):
    probs, rands, _ = corpus
    a = _run(opt, probs, rands)
    b = _run(opt, probs, rands)
    cap = max(max(p["n1"], p["n2"]) for p in probs)
    for k in range(len(probs)):
        for key in a[k]:
            assert a[k][key].tobytes() == b[k][key].tobytes(), (k, key)
    for k in (1, 8, 10, 16, len(probs) - 4, len(probs) - 2):
        one = _run(opt, [probs[k]], [rands[k]], cap=cap)[0]
        for key in one:
            assert one[key].tobytes() == a[k][key].tobytes(), (k, key)


def test_callers_stream(opt, corpus):
    probs, rands, oracle = corpus
    idx = [0, 10, 16]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run(opt, [probs[k] for k in idx], [rands[k] for k in idx], stream=s.cuda_stream)
    dev = []
    for j, k in enumerate(idx):
        _check(k, probs[k], got[j], oracle[k], dev)


def test_an_entry_beyond_the_second_frame_is_no_match(opt, corpus):
    """vnMatches12 entries at or beyond the second frame's count (the reference would read beyond mvKeys2) count as -1 on both sides."""
    probs, rands, oracle = corpus
    p = dict(probs[1])
    m = p["matches12"].copy()
    hit = np.nonzero(m >= 0)[0][[3, 40, 77]]
    m[hit] = [p["n2"], p["n2"] + 5, 2 ** 30]
    p["matches12"] = m
    o = two_view_oracle.run(p, rands[1])
    assert o["N"] == oracle[1]["N"] - 3
    _check("beyond", p, _run(opt, [p], [rands[1]])[0], o, [])
    q = dict(p, matches12=np.where(m >= p["n2"], -1, m).astype(np.int32))
    assert two_view_oracle.run(q, rands[1])["hyp"].tobytes() == o["hyp"].tobytes()


def test_invalid_arguments_are_refused_before_any_launch(opt):
    p = make_two_view_problem(0, n_matches=40, n1=60, n2=70)
    t = pack_two_view_problems([p], "cuda:0", rand=[libc_rand(1, 1600)])
    out = [torch.zeros(s, dtype=d, device="cuda:0") for s, d in (((1,), torch.int32), ((1, 12), torch.float32), ((1, 70, 3), torch.float32),
                                                                    ((1, 70), torch.uint8), ((1, len(TWO_VIEW_STATS)), torch.int32),
                                                                    ((1, len(TWO_VIEW_FSTATS)), torch.float32))]
    L = lib()

    def call(cap, max_it, rand_cap):
        return L.morb_two_view_reconstruction_batch(opt._h, 1, cap, ptr(t["img1"]), ptr(t["img2"]), ptr(t["count"]), ptr(t["kps"]),
                                                    ptr(t["matches12"]), ptr(t["K4"]), ptr(t["sigma"]), max_it, ptr(t["rand"]), rand_cap,
                                                    *[ptr(x) for x in out], None, None, None, None)
    assert call(70, 0, 1600) == ERR_INVALID
    assert call(70, 200, 1599) == ERR_INVALID
    assert call(0, 200, 1600) == ERR_INVALID
    torch.cuda.synchronize()
    assert all(not x.any() for x in out)   # nothing ran
    assert call(70, 200, 1600) == 0
    torch.cuda.synchronize()
    assert int(out[4][0, S["N"]]) == 40


def test_chain_from_search_for_initialization_on_one_stream(opt):
    """morb_search_for_initialization_batch -> morb_two_view_reconstruction_batch on one stream with no host copy in between, on one
    synthetic frame pair: the result equals the oracle run on the matcher's table, downloaded afterwards."""
    from morb_slam_amd import ORBmatcher
    from morb_slam_amd.capi import KP_DTYPE, make_frame_params
    p = make_two_view_problem(21, "general", n1=260, n2=250, n_matches=200, noise_px=0.3, outlier_frac=0.0)
    rng = np.random.default_rng(5)
    cap = 260
    # descriptors: a matched pair shares its 256 bits but for a few, every other keypoint is random
    d1 = rng.integers(0, 256, (p["n1"], 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (p["n2"], 32), dtype=np.uint8)
    m = p["matches12"]
    i1 = np.nonzero(m >= 0)[0]
    d2[m[i1]] = d1[i1] ^ (1 << rng.integers(0, 8, (len(i1), 32))).astype(np.uint8) * (rng.random((len(i1), 32)) < 0.1)
    kps = np.zeros((2, cap), KP_DTYPE)
    desc = np.zeros((2, cap, 32), np.uint8)
    for j, (kp, d, n) in enumerate(((p["kp1"], d1, p["n1"]), (p["kp2"], d2, p["n2"]))):
        kps[j, :n]["x"], kps[j, :n]["y"], kps[j, :n]["size"], kps[j, :n]["octave"] = kp[:, 0], kp[:, 1], 31.0, 0
        desc[j, :n] = d
    prev = np.zeros((1, cap, 2), np.float32)
    prev[0, :p["n1"]] = p["kp1"]
    params = make_frame_params(640, 480, float(p["K4"][0]), float(p["K4"][1]), float(p["K4"][2]), float(p["K4"][3]), 40.0, 0.08,
                               [1.0], [1.0])
    dev = "cuda:0"
    t_kps = torch.from_numpy(kps.view(np.uint8).reshape(2, cap, KP_DTYPE.itemsize).copy()).to(dev)
    t_desc, t_prev = torch.from_numpy(desc).to(dev), torch.from_numpy(prev).to(dev)
    count = torch.tensor([p["n1"], p["n2"]], dtype=torch.int32, device=dev)
    img1, img2 = torch.tensor([0], dtype=torch.int32, device=dev), torch.tensor([1], dtype=torch.int32, device=dev)
    rand = libc_rand(77, 1600)
    t_rand = torch.from_numpy(np.asarray(rand, np.int32)[None]).to(dev)
    K4, sigma = torch.from_numpy(p["K4"][None].copy()).to(dev), torch.ones(1, dtype=torch.float32, device=dev)
    matcher = ORBmatcher(0.9, True, device=0)
    try:
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            m12, nm = matcher.SearchForInitialization(params, img1, img2, t_kps, t_desc, count, t_prev, 100, stream=s.cuda_stream)
            out = opt.TwoViewReconstruction(img1, img2, count, t_kps, m12, K4, sigma, t_rand, 200, masks=True, hypScores=True,
                                            stream=s.cuda_stream)
        s.synchronize()
        table = m12.cpu().numpy()[0, :p["n1"]]
        assert int(nm[0]) >= 100 and (table >= 0).sum() == int(nm[0])
        o = two_view_oracle.run(dict(p, matches12=table), rand)
        g = {k: v.cpu().numpy()[0] for k, v in out.items()}
        dev_ = []
        _check("chain", p, g, o, dev_)
        assert o["ok"] == 1
    finally:
        matcher.close()
