"""Optimizer::OptimizeSim3 on the GPU (morb_optimize_sim3_batch) against the CPU oracle (tests/native/sim3_oracle.cc): one seeded batch of
problems covering both camera models on either side, free and fixed scale, 0 / 20 / 40 % outliers, matches outside KF2, bad points, matches
without pMP1, an early return, an empty problem and 15 .. 2000 matches; bAllPoints off in a second batch.  Batch == alone, rerun == rerun."""
import numpy as np
import pytest

import sim3_oracle
from morb_slam_amd.synth import make_sim3_problem, pack_sim3_problems

pytestmark = pytest.mark.gpu

FIELDS = ("entry", "Xw1", "Xw2", "i2", "obs1", "inv1", "obs2", "inv2")


def _specs():
    s = []
    for k, of in enumerate((0.0, 0.2, 0.4)):
        s.append(dict(n=300 + 50 * k, cam1="pinhole", cam2="pinhole", fix_scale=False, outlier_frac=of, noise_px=0.3))
        s.append(dict(n=250 + 40 * k, cam1="pinhole", cam2="pinhole", fix_scale=True, outlier_frac=of, noise_px=0.3))
        s.append(dict(n=200 + 30 * k, cam1="kb8", cam2="kb8", outlier_frac=of, noise_px=0.3))
    s += [dict(n=400, cam1="kb8", cam2="pinhole", outlier_frac=0.2, noise_px=0.3),
          dict(n=400, cam1="pinhole", cam2="kb8", outlier_frac=0.2, noise_px=0.3, fix_scale=True),
          dict(n=500, neg_i2_frac=0.2, bad_frac=0.1, no_mp1_frac=0.1, outlier_frac=0.2, noise_px=0.3),
          dict(n=500, neg_i2_frac=0.3, fix_scale=True, noise_px=0.3),
          dict(n=2000, outlier_frac=0.2, noise_px=0.5),
          dict(n=2000, cam1="kb8", cam2="kb8", outlier_frac=0.1, noise_px=0.5),
          dict(n=15, outlier_frac=0.0, unmatched_frac=0.0),
          dict(n=15, outlier_frac=0.5, unmatched_frac=0.0, noise_px=0.3),        # early return
          dict(n=20, unmatched_frac=1.0),                                           # empty: no match at all
          dict(n=100, no_mp1_frac=1.0),                                             # no correspondence: only matches without pMP1
          dict(n=60, bad_frac=0.3, outlier_frac=0.1, noise_px=0.3),
          dict(n=800, perturb=False, noise_px=0.2),
          dict(n=1000, cam1="kb8", cam2="pinhole", neg_i2_frac=0.1, bad_frac=0.05, noise_px=0.4),
          dict(n=120, cam1="pinhole", cam2="kb8", outlier_frac=0.4, noise_px=0.3),
          dict(n=600, cam1="kb8", cam2="kb8", fix_scale=True, outlier_frac=0.4, noise_px=0.3)]
    return s


def _problems(specs, seed0):
    out = []
    for k, sp in enumerate(specs):
        sp = dict(sp)
        n = sp.pop("n")
        out.append(make_sim3_problem(n, seed=seed0 + k, **sp))
    return out


def _run(opt, probs, bAllPoints):
    import torch
    t = pack_sim3_problems(probs, "cuda:0")
    nIn, keep, stats = opt.OptimizeSim3(t["entry"], t["Xw1"], t["Xw2"], t["i2"], t["obs1"], t["inv1"], t["obs2"], t["inv2"], t["T1w"], t["T2w"],
                                        t["cam1"], t["cam2"], t["th2"], t["fix"], t["S12"], bAllPoints=bAllPoints, count=t["count"])
    torch.cuda.synchronize()
    return nIn.cpu().numpy(), keep.cpu().numpy(), t["S12"].cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd.optimizer import Optimizer
    o = Optimizer(0)
    yield o
    o.close()


def _check_against_oracle(probs, specs, res, bAllPoints):
    """Every problem: return value, keep flags, reached-the-end flag and edge counts equal to the oracle's.  Pinhole pairs: also the LM
    iterations and trials of both phases, S12 within 1e-6.  A KannalaBrandt8 camera on either side: S12 within 1e-4, the LM path printed."""
    nIn, keep, S, stats = res
    kb8_paths = []
    for k, p in enumerate(probs):
        n = p["n"]
        o_nIn, o_keep, o_S, o_st = sim3_oracle.solve(p, bAllPoints)
        tag = f"problem {k} {specs[k]}"
        assert nIn[k] == o_nIn, tag
        assert (keep[k, :n] == o_keep).all(), tag
        assert (keep[k, n:] == 0).all(), tag
        assert stats[k, 4] == o_st[4], tag
        assert (stats[k, 5:] == o_st[5:]).all(), tag
        kb8 = p["cam1"][0] != 0 or p["cam2"][0] != 0
        tol = 1e-4 if kb8 else 1e-6
        if not kb8:
            assert (stats[k, :4] == o_st[:4]).all(), (tag, stats[k], o_st)
        else:
            kb8_paths.append((k, stats[k, :4].tolist(), o_st[:4].tolist()))
        qa, qb = S[k, :4], o_S[:4]
        assert min(np.abs(qa - qb).max(), np.abs(qa + qb).max()) <= tol, tag
        assert abs(S[k, 7] - o_S[7]) <= tol, tag
        assert np.abs(S[k, 4:7] - o_S[4:7]).max() <= tol * max(1.0, np.abs(o_S[4:7]).max()), tag
        if not o_st[4]:
            assert S[k].tobytes() == p["S12"].tobytes(), tag
    print("KB8 LM paths (problem, device its/trials, oracle its/trials):", kb8_paths)


def test_sim3_batch_matches_oracle(opt):
    specs = _specs()
    probs = _problems(specs, 100)
    assert len(probs) >= 24 and min(p["n"] for p in probs) == 15 and max(p["n"] for p in probs) == 2000
    res = _run(opt, probs, True)
    _check_against_oracle(probs, specs, res, True)
    st = res[3]
    assert st[:, 4].sum() >= 20 and (st[:, 4] == 0).sum() >= 3       # early returns and empty problems are in the batch
    # rerun: bit-identical
    res2 = _run(opt, probs, True)
    for a, b in zip(res, res2):
        assert a.tobytes() == b.tobytes()
    # each problem alone == its row of the batch, bit for bit
    for k, p in enumerate(probs):
        one = _run(opt, [p], True)
        n = p["n"]
        assert one[0][0] == res[0][k] and one[1][0, :n].tobytes() == res[1][k, :n].tobytes(), k
        assert one[2][0].tobytes() == res[2][k].tobytes() and one[3][0].tobytes() == res[3][k].tobytes(), k


def test_sim3_without_all_points(opt):
    specs = [dict(n=400, neg_i2_frac=0.3, outlier_frac=0.2, noise_px=0.3), dict(n=300, neg_i2_frac=0.5, fix_scale=True, noise_px=0.3),
             dict(n=300, cam1="kb8", cam2="kb8", neg_i2_frac=0.3, noise_px=0.3), dict(n=40, neg_i2_frac=0.9, noise_px=0.3)]
    probs = _problems(specs, 300)
    res = _run(opt, probs, False)
    _check_against_oracle(probs, specs, res, False)
    res_all = _run(opt, probs, True)
    assert (res[3][:3, 5] < res_all[3][:3, 5]).all()     # fewer correspondences without the points outside KF2


def _write_adapter_problem(path, p, bAllPoints, track_level=5):
    """One make_sim3_problem as tests/native/sim3_adapter_check.cc reads it: keyframes of mock keypoints whose octaves carry p's inverse sigmas;
    every pMP2 outside KF2 gets mnTrackScaleLevel = track_level (the reference reads level 0 there, not this one)."""
    n = p["n"]
    inv_level = ((1.0 / (1.2 ** np.arange(8)) ** 2)).astype(np.float32)
    octave = lambda inv: int(np.argmin(np.abs(inv_level - inv)))
    i2 = p["i2"]
    N2 = int(max(i2.max(initial=-1) + 1, 1))
    kp2 = np.zeros((N2, 2), np.float32); oct2 = np.zeros(N2, np.int32)
    for i in range(n):
        if i2[i] >= 0:
            kp2[i2[i]] = p["obs2"][i]; oct2[i2[i]] = octave(p["inv2"][i])
    kind = lambda c: int(c[0] != 0)
    with open(path, "wb") as f:
        f.write(np.array([n, N2, kind(p["cam1"]), kind(p["cam2"]), int(p["fix_scale"]), int(bAllPoints)], np.int32).tobytes())
        f.write(np.float32(p["th2"]).tobytes())
        for a in (p["cam1"][1:], p["cam2"][1:], p["T1w"], p["T2w"], inv_level):
            f.write(np.asarray(a, np.float32).tobytes())
        f.write(np.asarray(p["S12"], np.float64).tobytes())
        for i in range(n):
            f.write(np.uint8(p["entry"][i]).tobytes() + np.int32(i2[i]).tobytes() + p["Xw1"][i].astype(np.float32).tobytes() +
                    p["Xw2"][i].astype(np.float32).tobytes() + p["obs1"][i].astype(np.float32).tobytes() +
                    np.array([octave(p["inv1"][i]), track_level], np.int32).tobytes())
        for j in range(N2):
            f.write(kp2[j].tobytes() + np.int32(oct2[j]).tobytes())
    # the Python path's inputs are what the reference reads: KF2 sigmas of octave 0 for i2 < 0
    q = dict(p)
    q["inv1"] = inv_level[[octave(v) for v in p["inv1"]]]
    q["inv2"] = np.where(i2 >= 0, inv_level[[octave(v) for v in p["inv2"]]], inv_level[0]).astype(np.float32)
    return q


def test_reference_signature_member_on_gpu(opt, tmp_path):
    """The member template with the reference's signature, driven from C++ with mock keyframes (tests/native/sim3_adapter_check.cc): the same
    return value, vpMatches1 and g2oS12 as the Python path, mAcumHessian zeroed exactly when the function reaches its end."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nat = os.path.join(root, "tests", "native")
    libdir = os.path.join(root, "morb_slam_amd")
    exe = str(tmp_path / "sim3_adapter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(nat, "mock_ref"), "-I" + os.path.join(nat, "mock_sim3"),
                           "-I" + os.path.join(root, "include", "morb"), "-I" + os.path.join(root, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(nat, "sim3_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cases = [(dict(n=300, neg_i2_frac=0.2, bad_frac=0.05, no_mp1_frac=0.05, outlier_frac=0.2, noise_px=0.3), True),
             (dict(n=250, cam1="kb8", cam2="pinhole", fix_scale=True, neg_i2_frac=0.1, outlier_frac=0.1, noise_px=0.3), True),
             (dict(n=200, cam1="kb8", cam2="kb8", neg_i2_frac=0.3, noise_px=0.3), False),
             (dict(n=15, outlier_frac=0.5, unmatched_frac=0.0, noise_px=0.3), True)]      # early return
    reached = []
    for k, (sp, allp) in enumerate(cases):
        sp = dict(sp)
        p = make_sim3_problem(sp.pop("n"), seed=500 + k, **sp)
        fin, fout = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
        q = _write_adapter_problem(fin, p, allp)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
        n = p["n"]
        ret = int(np.frombuffer(raw[:4], np.int32)[0])
        vp = np.frombuffer(raw[4:4 + n], np.uint8)
        S = np.frombuffer(raw[4 + n:4 + n + 64], np.float64)
        hstate = int(np.frombuffer(raw[4 + n + 64:], np.int32)[0])
        nIn, keep, S_py, st = _run(opt, [q], allp)
        assert ret == nIn[0], (k, ret, nIn[0])
        assert (vp == keep[0, :n]).all(), k
        assert S.tobytes() == S_py[0].tobytes(), k
        assert hstate == (1 if st[0, 4] else 0), (k, hstate, st[0])
        if not st[0, 4]:
            assert S.tobytes() == np.asarray(p["S12"], np.float64).tobytes(), k
        reached.append(int(st[0, 4]))
    assert reached.count(1) >= 2 and reached.count(0) >= 1
