"""ORB_SLAM3::MLPnPsolver in the reference's signature (include/morb/MLPnPsolver.h), driven from C++ with a mock frame and map points
after srand(seed) (tests/native/mlpnp_solver_adapter_check.cc) in Tracking::Relocalization's loop shape: several candidates of one
frame, iterate(5, ..) round-robin, a candidate discarded on bNoMore; then one direct call.  Every call equals the CPU oracle fed the
rand() values that call drew (libc_rand(seed) in call order: minSet per iteration, for every iteration the call may run): the return
value, bNoMore, nInliers, vbInliers (empty unless true) and Tout within the project's pose gate 1e-4.  The program makes one throw-away
call before srand(seed): without it the first poses came out as if the stream had been moved between srand(seed) and the later draws
(suspected, not isolated: the HIP runtime starting up inside the first call); it also writes the next rand() value after the loop, so a
stream that does not stand where the oracle's does fails by itself."""
import os
import subprocess

import numpy as np
import pytest

import mlpnp_solver_oracle
from morb_slam_amd.synth import libc_rand, make_mlpnp_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LEV = ((1.2 ** np.arange(8)) ** 2).astype(np.float32)
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
ROUNDS = 3


def _candidates():
    """One frame (the keypoints of one generated scene) and five candidates' matches to it."""
    base = make_mlpnp_problem(220, seed=900, outlier_frac=0.0, bad_frac=0.0, unmatched_frac=0.0, noise_px=0.4)
    n_keys = 200                                    # mvKeysUn.size(): the last 20 features of a longer match vector are beyond it
    octave = np.array([int(np.argmin(np.abs(LEV - s))) for s in base["sigma2"]], np.int32)
    rng = np.random.default_rng(901)
    cands = []
    for n, of, unmatched, bad, extra in ((200, 0.2, 0.1, 0.05, {}), (220, 0.3, 0.0, 0.0, {}), (200, 0.9, 0.0, 0.0, {}),
                                         (200, 0.1, 0.96, 0.0, {}), (180, 0.45, 0.1, 0.0, dict(epsilon=0.4, min_set=8))):
        p = dict(base)
        p.update(n=n, **extra)
        Xw = base["Xw"][:n].astype(np.float64).copy()
        out = rng.random(n) < of
        Xw[out] += rng.normal(0, 0.6, (int(out.sum()), 3))
        matched = rng.random(n) >= unmatched
        isbad = rng.random(n) < bad
        beyond = np.arange(n) >= n_keys
        p["Xw"] = Xw.astype(np.float32)
        p["entry"] = (matched.astype(np.uint8) | (isbad.astype(np.uint8) << 1) | (beyond.astype(np.uint8) << 2)).astype(np.uint8)
        p["uv"], p["sigma2"] = base["uv"][:n].copy(), LEV[octave[:n]]
        cands.append(p)
    return base, octave, n_keys, cands


def _write(path, base, octave, n_keys, cands, seed):
    with open(path, "wb") as f:
        f.write(np.array([len(cands), seed, ROUNDS, int(base["cam"][0] != 0)], np.int32).tobytes())
        f.write(np.asarray(base["cam"][1:], np.float32).tobytes() + LEV.tobytes() + np.int32(n_keys).tobytes())
        for i in range(n_keys):
            f.write(base["uv"][i].astype(np.float32).tobytes() + np.int32(octave[i]).tobytes())
        for p in cands:
            f.write(np.array([p["n"], p["min_inliers"], p["max_iterations"], p["min_set"]], np.int32).tobytes())
            f.write(np.float64(p["probability"]).tobytes() + np.array([p["epsilon"], p["th2"]], np.float32).tobytes())
            for i in range(p["n"]):
                f.write(np.uint8(p["entry"][i] & 3).tobytes() + p["Xw"][i].astype(np.float32).tobytes())


def _read(path, cands):
    raw = open(path, "rb").read()
    out, off = [], 0
    while off < len(raw):
        cand, ok, noMore, nIn, size = np.frombuffer(raw[off:off + 20], np.int32); off += 20
        if cand < 0:   # the marker after the loop: the next rand() value
            out.append(dict(cand=-1, next_rand=int(ok)))
            continue
        n = cands[cand]["n"]
        vb = np.frombuffer(raw[off:off + n], np.uint8); off += n
        T = np.frombuffer(raw[off:off + 64], np.float32); off += 64
        out.append(dict(cand=int(cand), ok=int(ok), noMore=int(noMore), nInliers=int(nIn), size=int(size), mask=vb, T=T))
    assert off == len(raw)
    return out


class _Stream:
    """libc's rand() after srand(seed), consumed the way the adapter does: per call, minSet values for every iteration it may run."""

    def __init__(self, seed, cands):
        self.values, self.pos = libc_rand(seed, 40000), 0
        self.rand = [np.zeros(p["min_set"] * (p["max_iterations"] + 5 * ROUNDS + 5), np.int32) for p in cands]
        self.its = [0] * len(cands)
        self.calls = [0] * len(cands)

    def call(self, k, p):
        N, min_inl, budget = (lambda s: (s["N"], s["minInliers"], s["budget"]))(mlpnp_solver_oracle.run(p, self.rand[k], calls=[0])[1])
        it0 = self.its[k]
        end = max(budget, it0 + 5) if N >= min_inl else it0
        m = p["min_set"]
        cnt = (end - it0) * m
        self.rand[k][it0 * m:end * m] = self.values[self.pos:self.pos + cnt]
        self.pos += cnt
        self.calls[k] += 1
        o = mlpnp_solver_oracle.run(p, self.rand[k], calls=[5] * self.calls[k], stop=False)[0][-1]
        self.its[k] = o["iterations"]
        return o


def _same(a, o, k):
    assert (a["ok"], a["noMore"], a["nInliers"]) == (o["ok"], o["noMore"], o["nInliers"]), (k, a, o)
    if o["ok"]:
        assert a["size"] == len(o["mask"]) and np.array_equal(a["mask"], o["mask"]), k
        assert np.abs(a["T"] - o["Tcw"]).max() <= 1e-4, k
    else:
        assert a["size"] == 0 and not a["mask"].any() and np.array_equal(a["T"], IDENTITY), k


def test_reference_signature_class_on_gpu(tmp_path):
    exe = str(tmp_path / "mlpnp_solver_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_mlpnp_solver"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(NATIVE, "mlpnp_solver_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    base, octave, n_keys, cands = _candidates()
    seed = 5150
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write(fin, base, octave, n_keys, cands, seed)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read(fout, cands)
    loop, marker, direct = got[:-2], got[-2], got[-1]
    assert marker["cand"] == -1
    # the loop: round-robin over the candidates not yet discarded
    st = _Stream(seed, cands)
    discarded = [False] * len(cands)
    j = 0
    for _ in range(ROUNDS):
        for k, p in enumerate(cands):
            if discarded[k]:
                continue
            a = loop[j]; j += 1
            assert a["cand"] == k
            o = st.call(k, p)
            _same(a, o, (k, j))
            discarded[k] = bool(o["noMore"])
    assert j == len(loop)
    assert marker["next_rand"] == int(st.values[st.pos])   # the loop drew exactly the values the oracle was fed
    assert sum(a["ok"] for a in loop) >= 3 and sum(discarded) >= 2 and not all(discarded)
    assert any(a["ok"] and a["cand"] == 1 and not a["mask"][n_keys:].any() for a in loop)   # features beyond mvKeysUn are never inliers
    # the direct call: a fresh solver on the first candidate after srand(seed)
    _same(direct, _Stream(seed, cands).call(0, cands[0]), "direct")
