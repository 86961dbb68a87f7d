"""GPU parity of the device-resident LM optimisers against the CPU oracle (g2o semantics restated).
Tolerance from BASELINE.json north_star: <= 1e-4 on optimised poses (and points); outlier / erase flags and
inlier counts must be identical on these synthetic problems (no observation sits on a chi2 gate)."""
import numpy as np
import pytest

import oracle_lib as O
from morb_slam_amd.synth import make_ba_problem, make_pose_problem

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4


def _run_pose_batch(problems, exact=True):
    import torch
    from morb_slam_amd import Optimizer
    cap = max(len(p["hasMP"]) for p in problems)
    F = len(problems)
    has = np.zeros((F, cap), np.uint8); obs = np.zeros((F, cap, 3), np.float32); inv = np.ones((F, cap), np.float32)
    Xw = np.zeros((F, cap, 3), np.float32); pose = np.zeros((F, 7), np.float32); cnt = np.zeros(F, np.int32)
    for f, p in enumerate(problems):
        n = len(p["hasMP"]); cnt[f] = n
        has[f, :n] = p["hasMP"]; obs[f, :n] = p["obs"]; inv[f, :n] = p["invSigma2"]; Xw[f, :n] = p["Xw"]; pose[f] = p["pose0"]
    t = [torch.from_numpy(a).cuda() for a in (has, obs, inv, Xw, pose, cnt)]
    opt = Optimizer()
    opt.set_exact_order(exact)
    nin, outl, stats = opt.PoseOptimization(t[0], t[1], t[2], t[3], t[4], problems[0]["cam"], count=t[5])
    torch.cuda.synchronize()
    return nin.cpu().numpy(), outl.cpu().numpy(), stats.cpu().numpy(), t[4].cpu().numpy()


def test_pose_optimization_matches_oracle():
    probs = [make_pose_problem(600, seed=s) for s in range(6)]
    probs += [make_pose_problem(1200, seed=10, outlier_frac=0.3), make_pose_problem(60, seed=11, mono_frac=1.0),
              make_pose_problem(300, seed=12, mono_frac=0.0, rot_deg=5.0, trans=0.2)]
    nin, outl, stats, pose = _run_pose_batch(probs)
    for f, p in enumerate(probs):
        r, pe, oe, se = O.pose_optimization(p)
        n = len(p["hasMP"])
        assert np.abs(pose[f] - pe).max() <= POSE_TOL, (f, pose[f], pe)
        assert nin[f] == r
        np.testing.assert_array_equal(outl[f, :n], oe)
        # same LM trajectory, decision for decision: outer iterations AND trials.  Near convergence rho = dChi2 / scale is ~0 and its sign
        # follows the last bits of the sums over the edges (SURVEY "hard parts" 6): the kernel adds them in edge order like g2o / the oracle
        # (k_pose_opt<.., ORDERED>: the optimizer's deterministic mode, morb_optimizer_set_exact_order(1)); the default tree sums are checked below
        assert int(stats[f][0]) == int(se[0]) and int(stats[f][1]) == int(se[1]), (stats[f], se)
        assert np.abs(pose[f] - p["true"]).max() < 0.02   # and it actually converged to the truth


def test_edge_order_sums_on_the_matrix_core_equal_the_vector_chain(monkeypatch):
    """The edge-order sums run on v_mfma_f64_4x4x4_4b_f64 (four terms per instruction, added one after the other: optimizer.hip
    `ordered_add_mfma1`, tools/micro/mfma_chain.hip) when the device passes the self-test of morb_optimizer_create, on dependent v_add_f64
    otherwise.  Same order, same roundings: every output BIT of the two forms is equal — poses, flags, iteration and trial counts — at
    edge counts on both sides of the stage boundaries (po2_stage / po2_rows: 512 edges in the first stage, 384 in the later ones, batches of
    16 rows).  morb_optimizer_info must say which form each handle runs, and on this device the self-test must PASS: a rejected device is a
    failure here, not a skip (the default would silently be the slower vector chain)."""
    import torch
    from morb_slam_amd import Optimizer
    sizes = [40, 447, 448, 449, 463, 465, 511, 512, 513, 527, 529, 600, 767, 768, 769, 895, 896, 897, 1087, 1088, 1089, 1200, 1279, 1280, 1407, 1408, 1409, 1500, 1664]
    probs = [make_pose_problem(n, seed=100 + i) for i, n in enumerate(sizes)]
    for p in probs[:-4]:
        p["hasMP"][:] = 1          # the first round's edge count IS the size (later rounds drop the outliers: other counts)
    cap = max(len(p["hasMP"]) for p in probs)
    pad = lambda a: np.pad(a, [(0, cap - len(a))] + [(0, 0)] * (a.ndim - 1))
    t = [torch.from_numpy(np.stack([pad(p[k]) for p in probs])).cuda() for k in ("hasMP", "obs", "invSigma2", "Xw")]
    pose0 = torch.from_numpy(np.stack([p["pose0"] for p in probs])).cuda()
    cnt = torch.tensor([len(p["hasMP"]) for p in probs], dtype=torch.int32, device="cuda")
    res = {}
    for form in ("valu", "mfma", ""):
        if form:
            monkeypatch.setenv("MORB_PO2_CHAIN", form)
        else:
            monkeypatch.delenv("MORB_PO2_CHAIN")      # the handle decides by its self-test
        opt = Optimizer()
        opt.set_exact_order(True)
        want = {"valu": {"mfma_chain": 0, "exact_order": 1, "mfma_selftest": -1}, "mfma": {"mfma_chain": 1, "exact_order": 1, "mfma_selftest": -1},
                "": {"mfma_chain": 1, "exact_order": 1, "mfma_selftest": 1}}[form]
        assert opt.info() == want, (form, opt.info())
        pose = pose0.clone()
        nin, outl, stats = opt.PoseOptimization(t[0], t[1], t[2], t[3], pose, probs[0]["cam"], count=cnt)
        torch.cuda.synchronize()
        res[form] = (nin.cpu().numpy(), outl.cpu().numpy(), stats.cpu().numpy(), pose.cpu().numpy().view(np.uint32))
        opt.set_exact_order(False)
        assert opt.info()["exact_order"] == 0
    for a, b in zip(res["valu"], res["mfma"]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(res["mfma"], res[""]):            # MI355X passes the self-test: the default IS the matrix-core form
        np.testing.assert_array_equal(a, b)
    for f in (0, 2, 7, 13, 19, 25):                   # and both equal the oracle's LM path
        r, pe, oe, se = O.pose_optimization(probs[f])
        assert res["mfma"][0][f] == r and int(res["mfma"][2][f][0]) == int(se[0]) and int(res["mfma"][2][f][1]) == int(se[1])
        np.testing.assert_array_equal(res["mfma"][1][f, :sizes[f]], oe)


@pytest.mark.parametrize("n", [1700, 2100, 4000])
def test_pose_optimization_of_large_frames(n):
    """Frames with more active edges than the threads' registers hold (1664 in the edge-order mode, 2048 with tree sums) run the large-frame
    instantiation of k_pose_opt2: the further stages read their edge again in every pass.  Same LM path as the oracle in the edge-order mode."""
    probs = [make_pose_problem(n, seed=200 + n + s) for s in range(2)]
    for p in probs:
        p["hasMP"][:] = 1
    nin, outl, stats, pose = _run_pose_batch(probs)
    nin_t, outl_t, stats_t, pose_t = _run_pose_batch(probs, exact=False)
    for f, p in enumerate(probs):
        r, pe, oe, se = O.pose_optimization(p)
        assert np.abs(pose[f] - pe).max() <= POSE_TOL and np.abs(pose_t[f] - pe).max() <= POSE_TOL
        assert nin[f] == r and nin_t[f] == r
        np.testing.assert_array_equal(outl[f, :n], oe)
        np.testing.assert_array_equal(outl_t[f, :n], oe)
        assert int(stats[f][0]) == int(se[0]) and int(stats[f][1]) == int(se[1]), (stats[f], se)
        assert int(stats_t[f][0]) == int(se[0]) and abs(int(stats_t[f][1]) - int(se[1])) <= 2


def test_pose_optimization_tree_sum_mode():
    """The default (morb_optimizer_set_exact_order(0)): tree sums — same poses, flags and outer iterations; the trial count may differ by the
    rare flip of a ~0 rho (observed: 50 vs 49 in one of nine problems)."""
    import torch
    from morb_slam_amd import Optimizer
    probs = [make_pose_problem(600, seed=s) for s in range(6)] + [make_pose_problem(1200, seed=10, outlier_frac=0.3)]
    cap = max(len(p["hasMP"]) for p in probs)
    pad = lambda a: np.pad(a, [(0, cap - len(a))] + [(0, 0)] * (a.ndim - 1))
    t = [torch.from_numpy(np.stack([pad(p[k]) for p in probs])).cuda() for k in ("hasMP", "obs", "invSigma2", "Xw")]
    pose = torch.from_numpy(np.stack([p["pose0"] for p in probs])).cuda()
    cnt = torch.tensor([len(p["hasMP"]) for p in probs], dtype=torch.int32, device="cuda")
    opt = Optimizer()
    opt.set_exact_order(False)
    nin, outl, stats = opt.PoseOptimization(t[0], t[1], t[2], t[3], pose, probs[0]["cam"], count=cnt)
    torch.cuda.synchronize()
    for f, p in enumerate(probs):
        r, pe, oe, se = O.pose_optimization(p)
        assert np.abs(pose[f].cpu().numpy() - pe).max() <= POSE_TOL and int(nin[f]) == r
        np.testing.assert_array_equal(outl[f, :len(oe)].cpu().numpy(), oe)
        assert int(stats[f][0]) == int(se[0]) and abs(int(stats[f][1]) - int(se[1])) <= 2


def test_pose_optimization_degenerate():
    few = make_pose_problem(40, seed=20)
    few["hasMP"][:] = 0; few["hasMP"][:2] = 1          # < 3 correspondences -> returns 0, pose untouched (:951)
    eight = make_pose_problem(40, seed=21)
    eight["hasMP"][:] = 0; eight["hasMP"][:8] = 1      # < 10 edges -> a single round (:1039)
    nin, outl, stats, pose = _run_pose_batch([few, eight])
    assert nin[0] == 0 and np.array_equal(pose[0], few["pose0"])
    r, pe, oe, se = O.pose_optimization(eight)
    assert nin[1] == r and np.abs(pose[1] - pe).max() <= POSE_TOL and int(stats[1][1]) == int(se[1])


@pytest.mark.parametrize("kw", [dict(seed=1), dict(seed=2, n_free=8, n_fixed=3, n_points=500),
                                dict(seed=3, n_free=20, n_fixed=6, n_points=3000, mono_frac=0.5)])
def test_local_ba_matches_oracle(kw):
    from morb_slam_amd import Optimizer
    b = make_ba_problem(**kw)
    opt = Optimizer()
    for inertial, mode in ((False, 0), (True, 0), (False, 1), (True, 1)):   # grid mode and persistent-workgroup mode
        kf, mp, erase, stats = opt.LocalBundleAdjustment(b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"],
                                                         b["eInvSigma2"], b["cam"], inertial=inertial, mode=mode)
        its, kfe, mpe, ee, se = O.local_ba(b, lambda100=inertial)
        assert int(stats[0]) == int(se[0]) and int(stats[1]) == int(se[1]), (stats, se)
        assert np.abs(kf - kfe).max() <= POSE_TOL
        assert np.abs(mp - mpe).max() <= 1e-4 * max(1.0, np.abs(mpe).max())
        np.testing.assert_array_equal(erase, ee)
        nf = int((b["kfFixed"] == 0).sum())
        assert np.abs(kf[:nf] - b["true_poses"][:nf]).max() < 0.05


@pytest.mark.parametrize("n_free", [30, 45, 60])
def test_local_ba_large_windows(n_free):
    """The reference takes EVERY covisible keyframe (Optimizer.cc:1058-1070, no cap): beyond 27 free keyframes the reduced camera system
    (6 n > 163 unknowns) no longer fits the LDS-resident LDL^T and is factorised in global memory, one 16-column panel in LDS at a time
    (dense_ldlt.h: ldlt_solve_global) — same LM path, poses / points within 1e-4, identical erase flags."""
    from morb_slam_amd import Optimizer
    b = make_ba_problem(seed=5, n_free=n_free, n_fixed=6, n_points=3000)
    opt = Optimizer()
    for inertial in (False, True):
        kf, mp, erase, stats = opt.LocalBundleAdjustment(b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"],
                                                         b["cam"], inertial=inertial, mode=0)
        its, kfe, mpe, ee, se = O.local_ba(b, lambda100=inertial)
        assert int(stats[0]) == int(se[0]) and int(stats[1]) == int(se[1]), (stats, se)
        assert np.abs(kf - kfe).max() <= POSE_TOL
        assert np.abs(mp - mpe).max() <= 1e-4 * max(1.0, np.abs(mpe).max())
        np.testing.assert_array_equal(erase, ee)
        assert np.abs(kf[:n_free] - b["true_poses"][:n_free]).max() < 0.05


def test_local_ba_stop_flag():
    from morb_slam_amd import Optimizer
    b = make_ba_problem(seed=4, n_free=5, n_fixed=2, n_points=200)
    for mode in (0, 1):
        kf, mp, erase, stats = Optimizer().LocalBundleAdjustment(b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"],
                                                                 b["eInvSigma2"], b["cam"], stop=True, mode=mode)
        assert stats.tolist() == [0, 0]                       # *pbStopFlag set: graph is not optimised (:1355)
        np.testing.assert_array_equal(kf, b["kfPose"])


def test_local_ba_abort_from_another_thread_while_solving():
    # LocalMapping::InterruptBA arrives on the tracking thread while LocalBundleAdjustment runs (LocalMapping.cc:884,
    # Optimizer.cc:1142): the persistent-workgroup solve (25 ms for the C5 graph) must stop early, on the handle's own stream
    import threading, time
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import BAProblem
    b = make_ba_problem(seed=3, n_free=20, n_fixed=6, n_points=3000, mono_frac=0.5)
    opt = Optimizer()
    p = BAProblem(opt, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    p.set_mode(1)
    p.solve(); full = p.results()[3].copy()        # undisturbed: the full schedule
    assert full[0] >= 3
    p.set_stop(False)
    t = threading.Thread(target=lambda: (time.sleep(0.003), p.set_stop(True)))
    t0 = time.perf_counter()
    p.solve(); t.start()
    kf, mp, erase, stats = p.results()
    dt = time.perf_counter() - t0
    t.join()
    assert stats[0] < full[0], (stats, full)       # fewer outer iterations than the undisturbed solve
    assert np.isfinite(kf).all() and np.isfinite(mp).all()
    p.set_stop(False)
    p.solve()
    assert p.results()[3].tolist() == full.tolist()  # the flag is a level, not sticky state


def test_local_ba_oneshot_polls_the_callers_flag():
    # the reference binding passes pbStopFlag itself (a one-byte bool): set at entry -> nothing optimised; set by another
    # thread during the grid-mode solve -> the host LM loop stops at the next iteration / trial
    import threading, time
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    b = make_ba_problem(seed=3, n_free=20, n_fixed=6, n_points=3000, mono_frac=0.5)
    opt = Optimizer()
    args = (b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    flag = np.zeros(4, np.uint8); flag[1:] = 255                 # neighbours of the bool must not be read as part of it
    full = local_bundle_adjustment_oneshot(opt, *args, stop_flag=flag[:1])[3]
    assert full[0] >= 3
    flag[0] = 1
    kf, mp, erase, stats = local_bundle_adjustment_oneshot(opt, *args, stop_flag=flag[:1])
    assert stats.tolist() == [0, 0]
    np.testing.assert_array_equal(kf, b["kfPose"])
    flag[0] = 0
    t = threading.Thread(target=lambda: (time.sleep(0.0015), flag.__setitem__(0, 1)))
    t.start()
    stats = local_bundle_adjustment_oneshot(opt, *args, stop_flag=flag[:1])[3]
    t.join()
    assert stats[1] <= full[1]


def test_local_ba_oneshot_equals_the_three_step_form():
    # the one-shot entry carves its problem from the handle's workspace and uploads it in one copy; the persistent form carves the same
    # layout from a block it owns: same kernels, same numbers — bit for bit — and the workspace is reused by the next call
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    opt = Optimizer()
    for kw in (dict(seed=1), dict(seed=2, n_free=8, n_fixed=3, n_points=500), dict(seed=1)):
        b = make_ba_problem(**kw)
        ref = opt.LocalBundleAdjustment(b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
        one = local_bundle_adjustment_oneshot(opt, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
        for x, y in zip(ref, one):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_a_tracking_search_does_not_wait_for_a_running_local_ba():
    """The reference runs Tracking and LocalMapping on two threads.  A projection search on a fresh matcher handle — whose first call GROWS its
    workspaces — must not wait for a LocalBundleAdjustment that is running on another handle: until round 5 the growth went through
    hipDeviceSynchronize + hipFree, i.e. it waited for the whole device.  The solve here is the persistent-workgroup mode (one kernel of tens of ms),
    started on one thread; the search runs to completion on another while the solve is still in flight."""
    import threading
    import time
    import torch
    from morb_slam_amd import BAProblem, Optimizer, ORBmatcher
    from morb_slam_amd.capi import make_frame_params
    from morb_slam_amd.synth import make_ba_problem
    opt = Optimizer()
    b = make_ba_problem(seed=2)
    p = BAProblem(opt, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    p.set_mode(1)
    p.solve(); p.results()                                   # warm (code objects loaded, buffers there)
    t0 = time.perf_counter(); p.solve(); p.results(); solve_s = time.perf_counter() - t0
    assert solve_s > 0.005, "the persistent solve is expected to take milliseconds"
    rng = np.random.default_rng(1)
    cap = mp = 512
    from morb_slam_amd import KP_DTYPE
    k = np.zeros((1, cap), KP_DTYPE); k["x"] = rng.uniform(20, 700, (1, cap)); k["y"] = rng.uniform(20, 440, (1, cap)); k["octave"] = rng.integers(0, 8, (1, cap))
    dev = "cuda"
    kps = torch.from_numpy(k.view(np.uint8).reshape(1, cap, 28)).to(dev)
    desc = torch.from_numpy(rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)).to(dev)
    cnt = torch.tensor([cap], dtype=torch.int32, device=dev)
    sf = [1.2 ** i for i in range(8)]
    P = make_frame_params(752, 480, 458.654, 457.296, 367.215, 248.375, 50.0, 0.11, sf, [s * s for s in sf])
    trk = dict(inView=torch.ones((1, mp), dtype=torch.uint8, device=dev), projX=torch.from_numpy(k["x"].astype(np.float32)).to(dev),
               projY=torch.from_numpy(k["y"].astype(np.float32)).to(dev), projXR=torch.full((1, mp), -1.0, device=dev),
               depth=torch.full((1, mp), 3.0, device=dev), level=torch.from_numpy(k["octave"].astype(np.int32)).to(dev),
               viewCos=torch.full((1, mp), 0.9, device=dev))
    z8 = torch.zeros((1, mp), dtype=torch.uint8, device=dev)
    fImg = torch.zeros((1,), dtype=torch.int32, device=dev); nMP = torch.tensor([mp], dtype=torch.int32, device=dev)
    ones8 = torch.ones_like(z8)
    matchF = torch.full((1, cap), -1, dtype=torch.int32, device=dev); nmOut = torch.zeros((1,), dtype=torch.int32, device=dev)
    # the search runs on a NON-BLOCKING stream, as a C++ caller's would (the adapters of include/morb/ never touch the null stream): the legacy
    # default stream — torch's current stream here — is ordered with every blocking stream, the solver's included, so nothing below may use it
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    done = {}

    NS = 8                                                   # solves queued back to back: the device is busy with them for NS x solve_s

    def solver():
        t = time.perf_counter()
        for _ in range(NS):
            p.solve()                                        # (persistent mode: the call returns once the kernel is queued)
        p.results(); done["solve"] = (t, time.perf_counter())
    th = threading.Thread(target=solver); th.start()
    time.sleep(solve_s * 0.5)                                # the first solve is in flight, seven more behind it
    t1 = time.perf_counter()
    m = ORBmatcher(0.8, True)                                # fresh handle: every workspace grows inside the call below
    mt, nm = m.SearchByProjectionMapPoints(P, fImg, kps, desc, cnt, None, z8, nMP, trk, z8, desc, ones8, 3.0, matchF=matchF, nm=nmOut,
                                           stream=side.cuda_stream)
    side.synchronize()
    t2 = time.perf_counter()
    th.join()
    assert int(nm[0]) > 100
    assert t2 < done["solve"][1], f"the search should have finished while the solve was still running (search {t1:.4f} .. {t2:.4f}, solve {done['solve']})"
    assert t2 - t1 < 0.5 * (NS - 1) * solve_s, f"the search took {t2 - t1:.4f} s beside {NS} solves of {solve_s:.4f} s: it waited for them"


def test_optimizer_workspace_growth_does_not_wait_for_another_handles_solve():
    """Optimizer.h:46-139 is all-static and entered from three threads.  The one-shot entry points carve their problem from the handle's grow-only
    workspace / pinned staging buffer (morb_optimizer_workspace / _staging); until round 6 OUTGROWING them went through hipStreamSynchronize + hipFree,
    and hipFree waits for the whole DEVICE — i.e. for a LocalBundleAdjustment another thread has running on another handle.  Now the outgrown buffers
    are retired and freed with the handle.  Here: eight persistent-mode solves (tens of ms each) are queued on one handle by one thread; meanwhile a
    second handle runs a small one-shot LocalBundleAdjustment (first growth, from nothing) and then one three times its size (outgrows both buffers):
    both must return while the other handle's solves are still in flight, with the results of an undisturbed run."""
    import threading
    import time
    import torch
    from morb_slam_amd import BAProblem, Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    from morb_slam_amd.synth import make_ba_problem
    opt = Optimizer()
    b = make_ba_problem(seed=2)
    p = BAProblem(opt, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    p.set_mode(1)
    p.solve(); p.results()
    t0 = time.perf_counter(); p.solve(); p.results(); solve_s = time.perf_counter() - t0
    assert solve_s > 0.005
    small = make_ba_problem(seed=3, n_free=6, n_fixed=3, n_points=600)
    large = make_ba_problem(seed=4, n_free=20, n_fixed=6, n_points=3000)
    args = lambda q: (q["kfPose"], q["kfFixed"], q["mpPos"], q["eKF"], q["eMP"], q["eObs"], q["eInvSigma2"], q["cam"])
    quiet = Optimizer()
    want = [local_bundle_adjustment_oneshot(quiet, *args(q)) for q in (small, large)]     # undisturbed (also loads the code objects)
    quiet.close()
    torch.cuda.synchronize()
    NS, done = 8, {}

    def solver():
        t = time.perf_counter()
        for _ in range(NS):
            p.solve()
        p.results(); done["solve"] = (t, time.perf_counter())
    th = threading.Thread(target=solver); th.start()
    time.sleep(solve_s * 0.5)
    fresh = Optimizer()
    t1 = time.perf_counter()
    got = [local_bundle_adjustment_oneshot(fresh, *args(small)), local_bundle_adjustment_oneshot(fresh, *args(large))]
    t2 = time.perf_counter()
    th.join()
    for g, w in zip(got, want):
        for a, c in zip(g, w):
            np.testing.assert_array_equal(a, c)
    assert t2 < done["solve"][1], f"both one-shot calls should have returned while the other handle's solves ran ({t1:.4f} .. {t2:.4f}, solves {done['solve']})"
    assert t2 - t1 < 0.5 * (NS - 1) * solve_s, f"the one-shot calls took {t2 - t1:.4f} s beside {NS} solves of {solve_s:.4f} s: they waited for them"
    fresh.close(); p.close(); opt.close()
