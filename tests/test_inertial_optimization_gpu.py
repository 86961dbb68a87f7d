"""Optimizer::InertialOptimization on the GPU (morb_inertial_optimization_batch) against the CPU oracle
(tests/native/inertial_optimization_oracle.cc: dense system, dense LDL^T).  Parity = the same LM / GN path (d_stats4 equal), velocities, biases
and Rwg entries within 1e-4 absolute, the scale within 1e-4 relative, d_reintegrate equal: the bar of tests/test_inertial_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import inertial_optimization_cases as cases
import inertial_optimization_oracle as io
from morb_slam_amd.synth import imu_calib_diagonals, pack_inertial_optimization_problems

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def opt():
    from morb_slam_amd import Optimizer
    o = Optimizer(0)
    yield o
    o.close()


def run_gpu(opt, probs, pres, mode, cap=None, pad_rows=0, fill=9):
    dev = torch.device("cuda", 0)
    ks, st, hl, pre, fl, pr, g16 = pack_inertial_optimization_problems(probs, pres, dev, pad_rows=pad_rows)
    K, P = st.shape[0], len(probs)
    out = (torch.full((K,), fill, dtype=torch.uint8, device=dev), torch.full((P, 4), -7, dtype=torch.int32, device=dev),
           torch.full((P, 2), -7.0, dtype=torch.float64, device=dev))
    if cap is None:
        cap = max(p["kfState"].shape[0] for p in probs)
    opt.InertialOptimization(ks, st, hl, pre, mode, fl, pr, g16, cap=cap, out=out)
    torch.cuda.synchronize()
    ks = ks.cpu().numpy()
    st, g16, re, stats, chi2 = (t.cpu().numpy() for t in (st, g16, out[0], out[1], out[2]))
    return [dict(kfState=st[ks[i]:ks[i + 1]], global16=g16[i], reintegrate=re[ks[i]:ks[i + 1]], stats=stats[i], chi2=chi2[i]) for i in range(P)], \
        dict(kfState=st, reintegrate=re)


def assert_parity(g, o, mode, tag):
    assert g["stats"].tolist() == o["stats"].tolist(), (tag, g["stats"], o["stats"])
    dv = np.abs(g["kfState"][:, 12:] - o["kfState"][:, 12:]).max()
    assert dv <= 1e-4, (tag, "velocities / biases", dv)
    assert np.array_equal(g["kfState"][:, :12], o["kfState"][:, :12]), (tag, "poses are read only")
    dR = np.abs(g["global16"][:9] - o["global16"][:9]).max()
    assert dR <= 1e-4, (tag, "Rwg", dR)
    assert abs(g["global16"][9] - o["global16"][9]) <= 1e-4 * abs(o["global16"][9]), (tag, "scale", g["global16"][9], o["global16"][9])
    db = np.abs(g["global16"][10:] - o["global16"][10:]).max()
    assert db <= 1e-4, (tag, "bg / ba", db)
    if mode != 2:
        assert np.array_equal(g["reintegrate"], o["reintegrate"]), tag
    assert np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9), (tag, g["chi2"], o["chi2"])


@pytest.mark.parametrize("n", cases.SMALL + cases.LARGE)
def test_mode0_parity(opt, n):
    """InertialOptimization(pMap, Rwg, scale, bg, ba, bMono, ..., bFixedVel, ..., priorG, priorA): mono and stereo, the three prior settings,
    bFixedVel; N = 192 keeps its chain in LDS, N = 193 (cap = N) in the global workspace."""
    keys = [c for c in cases.MODE0_CASES if c[0] == n and c not in cases.LEFT_OUT]
    assert keys
    sc = [cases.mode0_scene(*k) for k in keys]
    res, _ = run_gpu(opt, [p for p, _ in sc], [pre for _, pre in sc], 0, cap=n)
    for k, (p, pre), g in zip(keys, sc, res):
        assert_parity(g, cases.oracle(("m0",) + k, p, pre, 0), 0, k)
        assert g["stats"][2] == 1 and g["stats"][3] == n - 1


@pytest.mark.parametrize("n", [10, 300])
def test_mode1_parity(opt, n):
    """InertialOptimization(pMap, bg, ba, priorG, priorA): Rwg = I and scale = 1 whatever the array holds; those ten values stay bit for bit."""
    p, pre = cases.mode1_scene(n)
    p = dict(p)
    p["global16"] = p["global16"].copy()
    p["global16"][:10] = np.arange(10) * 0.37 + 0.11
    res, _ = run_gpu(opt, [p], [pre], 1)
    o = cases.oracle(("m1", n, "ten values given"), p, pre, 1)   # (a key of its own: ("m1", n) is the unmodified scene of the CPU tests)
    assert_parity(res[0], o, 1, n)
    assert res[0]["global16"][:10].tobytes() == p["global16"][:10].tobytes()
    assert o["global16"][:10].tobytes() == p["global16"][:10].tobytes()
    assert np.abs(res[0]["global16"][10:13] - p["bg_true"]).max() < 2e-3      # the gyro bias is what this call is for


@pytest.mark.parametrize("n,outliers", [(10, ()), (65, ()), (65, (7, 40))])
def test_mode2_parity(opt, n, outliers):
    """InertialOptimization(pMap, Rwg, scale): Gauss-Newton, Huber on every link (two gross-outlier links take its second branch); velocities and
    biases stay bit for bit."""
    p, pre = cases.mode2_scene(n, outliers=outliers)
    res, _ = run_gpu(opt, [p], [pre], 2)
    g, o = res[0], cases.oracle(("m2", n, outliers), p, pre, 2)
    assert_parity(g, o, 2, (n, outliers))
    assert g["kfState"].tobytes() == p["kfState"].tobytes()
    assert g["global16"][10:].tobytes() == p["global16"][10:].tobytes()
    assert g["reintegrate"].tolist() == [9] * n
    assert g["stats"].tolist() == [10, 0, 1, n - 1]
    assert g["chi2"][1] < g["chi2"][0]
    if outliers:   # the outlier links' errors at the result are far beyond what Huber's delta 1 leaves quadratic (information ~1e6 .. 1e9)
        e2 = [io.edge(pre[k], p["kfState"][k - 1], p["kfState"][k], p["kfState"][k - 1, 12:15], p["kfState"][k, 12:15], g["global16"])[0] for k in outliers]
        assert all(np.abs(e).max() > 0.05 for e in e2)


def test_broken_chain(opt):
    """d_hasLink = 0 in the middle of a 12-keyframe problem: two chains that only share the global unknowns."""
    p, pre = cases.scene(("broken", 12), n_kf=12, seed=5, mono=True, s_true=1.2, n_imu=20, broken=(6,))
    assert p["hasLink"].tolist() == [0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    res, _ = run_gpu(opt, [p], [pre], 0)
    assert_parity(res[0], cases.oracle(("broken", 12), p, pre, 0), 0, "broken")
    assert res[0]["stats"][3] == 10


MIXED = (3, 10, 1, 65, 11, 5, 33, 64)


def _mixed():
    sc = []
    for i, n in enumerate(MIXED):
        p, pre = cases.scene(("mixed", i, n), n_kf=max(n, 2), seed=40 + i, mono=bool(i & 1), s_true=1.2 if i & 1 else 1.0, n_imu=20)
        if n == 1:
            p = dict(p, kfState=p["kfState"][:1], hasLink=p["hasLink"][:1])
            pre = pre[:1]
        if i == 5:
            p = dict(p, hasLink=np.zeros(n, np.uint8))
        sc.append((p, pre))
    return sc


def test_mixed_batch_and_determinism(opt):
    """Eight problems of 1 to 65 keyframes in one batch: the one-keyframe problem and the one without a link get ok = 0 and keep their rows; every
    other problem equals its own single-problem run bit for bit; rows beyond the last problem stay; a second run is bit-identical."""
    sc = _mixed()
    probs, pres = [p for p, _ in sc], [pre for _, pre in sc]
    res, whole = run_gpu(opt, probs, pres, 0, cap=65, pad_rows=3)
    res2, whole2 = run_gpu(opt, probs, pres, 0, cap=65, pad_rows=3)
    for a, b in zip(res, res2):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert whole["kfState"].tobytes() == whole2["kfState"].tobytes()
    assert np.all(whole["kfState"][-3:] == np.float32(7.25)) and whole["reintegrate"][-3:].tolist() == [9, 9, 9]
    for i, ((p, pre), g) in enumerate(zip(sc, res)):
        if i in (2, 5):
            assert g["stats"].tolist() == [0, 0, 0, 0]
            assert g["kfState"].tobytes() == p["kfState"].tobytes() and g["global16"].tobytes() == p["global16"].tobytes()
            assert set(g["reintegrate"].tolist()) == {9} and g["chi2"].tolist() == [-7.0, -7.0]
            continue
        single, _ = run_gpu(opt, [p], [pre], 0)
        for k in g:
            assert g[k].tobytes() == single[0][k].tobytes(), (i, k)
        assert g["stats"][2] == 1


@pytest.mark.parametrize("offset,expect", [(0.05, 1), (0.001, 0)])
def test_reintegrate_flag(opt, offset, expect):
    """A true gyro bias 0.05 rad/s from the bias the links were integrated with flags every linked keyframe; 0.001 rad/s flags none."""
    p, pre = cases.scene(("reint", offset), n_kf=12, seed=7, mono=False, s_true=1.0, n_imu=20, gyro_bias_offset=offset, prior_g=1e2, prior_a=1e5)
    res, _ = run_gpu(opt, [p], [pre], 0)
    g = res[0]
    assert_parity(g, cases.oracle(("reint", offset), p, pre, 0), 0, offset)
    assert g["reintegrate"].tolist() == [0] + [expect] * 11
    assert np.abs(g["global16"][10:13] - p["bg_true"]).max() < 2e-3


def test_device_chain(opt):
    """morb_imu_preintegrate_batch -> morb_inertial_optimization_batch on one stream, no host copy in between; the result is the one of the
    run fed with the oracle's preintegrations."""
    dev = torch.device("cuda", 0)
    sc = [cases.mode0_scene(10, "mono", s) for s in range(3)]
    probs = [p for p, _ in sc]
    nga, walk = imu_calib_diagonals()
    off = np.cumsum([0] + [len(p["dt"]) for p in probs])
    start = np.concatenate([p["imuStart"][:-1] + o for p, o in zip(probs, off[:-1])] + [off[-1:]]).astype(np.int32)
    cat = lambda k: torch.from_numpy(np.concatenate([p[k] for p in probs])).to(dev)
    bias = torch.from_numpy(np.concatenate([np.tile(p["bias"], (p["kfState"].shape[0], 1)) for p in probs])).to(dev)
    ks, st, hl, _, fl, pr, g16 = pack_inertial_optimization_problems(probs, [pre for _, pre in sc], dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        pre_d = opt.PreintegrateIMU(torch.from_numpy(start).to(dev), cat("acc"), cat("gyro"), cat("dt"), bias, nga, walk, stream=s.cuda_stream)
        re, stats, chi2 = opt.InertialOptimization(ks, st, hl, pre_d, 0, fl, pr, g16, cap=10, stream=s.cuda_stream)
    s.synchronize()
    ref, _ = run_gpu(opt, probs, [pre for _, pre in sc], 0)
    st, g16, stats = st.cpu().numpy(), g16.cpu().numpy(), stats.cpu().numpy()
    for i, r in enumerate(ref):
        assert stats[i].tolist() == r["stats"].tolist()
        assert np.abs(st[10 * i:10 * i + 10] - r["kfState"]).max() <= 1e-4
        assert np.abs(g16[i] - r["global16"]).max() <= 1e-4


def test_cap_beyond_4096_is_refused(opt):
    from morb_slam_amd.capi import MorbError
    p, pre = cases.mode0_scene(3, "mono", 0)
    with pytest.raises(MorbError) as e:
        run_gpu(opt, [p], [pre], 0, cap=4097)
    assert e.value.code == -3      # MORB_ERR_CAPACITY


def test_reference_typed_member(opt, tmp_path):
    """Optimizer::InertialOptimization(Map*, Rwg, scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG, priorA) of
    include/morb/Optimizer_reference.h on mock keyframes (tests/native/inertial_optimization_member_check.cc): what it writes back — velocity
    and bias of every keyframe, the Reintegrate() calls, Rwg, scale, bg, ba — is what the view-taking call gives on the same arrays."""
    from test_adapter_gpu import ROOT
    p, pre = cases.scene(("member", 12), n_kf=12, seed=11, mono=True, s_true=1.2, n_imu=20, gyro_bias_offset=0.03)
    res, _ = run_gpu(opt, [p], [pre], 0)
    g = res[0]
    d = tmp_path / "io"
    d.mkdir()
    put = lambda name, a: np.ascontiguousarray(a).tofile(str(d / (name + ".bin")))
    put("kf_state", p["kfState"]); put("pre", pre.astype(np.float32)); put("global16", p["global16"]); put("prior2", p["prior2"])
    put("cfg", np.array([12, p["flags"]], np.int32))
    exe = str(tmp_path / "member_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tests", "native", "mock_inertial_optimization"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "inertial_optimization_member_check.cc"), "-L" + libdir, "-lmorb_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "inertial optimization member ok" in out.stdout, out.stdout + out.stderr
    get = lambda name, dt: np.fromfile(str(d / ("out_" + name + ".bin")), dtype=dt)
    vb = get("vel_bias", np.float32).reshape(12, 9)
    assert vb.tobytes() == np.ascontiguousarray(g["kfState"][:, 12:]).tobytes()
    assert get("reintegrated", np.int32).tolist() == g["reintegrate"].astype(np.int32).tolist()
    assert get("global16", np.float64).tobytes() == g["global16"].tobytes()
    # the second overload (bg, ba, priorG, priorA) and the third (Rwg, scale) ran too: their outputs are finite and the third moved nothing but Rwg / scale
    assert np.isfinite(get("global16_mode1", np.float64)).all() and np.isfinite(get("global16_mode2", np.float64)).all()
