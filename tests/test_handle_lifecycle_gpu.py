"""Handle life cycles release everything their handles hold (csrc/hip_owned.h).  Twenty cycles of: an extractor created, run at two sizes
(a reconfigure) and on one image through the host API, destroyed; a matcher run through a stereo match and a projection search (workspace
growth), destroyed; an optimizer running a create / solve / results / close BA problem, a one-shot LocalBA and a fisheye one-shot, destroyed.
The device's free memory after the last cycle stays within a bound of what it was after the first; one cycle's 1920 x 1080 extractor buffers
alone are several times that bound.  (Pinned host memory is not visible this way: tests/test_hip_resources_cpu.py covers its owners.)"""
import gc

import numpy as np
import pytest

from morb_slam_amd.synth import make_ba_problem, make_ba_problem_fisheye, make_stereo_pair

pytestmark = pytest.mark.gpu

CYCLES = 20
BOUND = 64 << 20                                   # bytes
MBF, MB = np.float32(458.654 * 0.11), np.float32(0.11)


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def _projection_search(m, kps, desc, cnt, ext, u):
    """isInFrustum + SearchByProjection(F, vpMapPoints) of frame 0's left keypoints, back-projected at their stereo depth, into the same image."""
    import torch
    from morb_slam_amd.capi import make_frame_params
    P = make_frame_params(752, 480, 458.654, 457.296, 367.215, 248.375, float(MBF), float(MB), ext.GetScaleFactors(),
                          ext.GetScaleSigmaSquares())
    n0 = int(cnt[0])
    k0 = kps[0, :n0].cpu().numpy().view(np.float32)                 # [n0, 7]: x, y, size, angle, response, octave, class_id
    ur = u[0, :n0].cpu().numpy()
    z = np.where(ur > 0, float(MBF) / np.maximum(k0[:, 0] - ur, 1e-3), 5.0).astype(np.float32)
    Xw = np.stack([(k0[:, 0] - P.cx) * z / P.fx, (k0[:, 1] - P.cy) * z / P.fy, z], 1).astype(np.float32)
    n = len(Xw)
    dist = np.linalg.norm(Xw, axis=1).astype(np.float32)
    normal = (Xw / dist[:, None]).astype(np.float32)
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)[None]).to(dev)
    nMP = torch.tensor([n], dtype=torch.int32, device=dev)
    trk = m.isInFrustum(P, t(np.eye(3, dtype=np.float32).reshape(9)), t(np.zeros(3, np.float32)), t(np.zeros(3, np.float32)), nMP,
                        t(Xw), t(normal), t(dist * 2), t(dist / 4), 0.5)
    cap = kps.shape[1]
    fImg = torch.tensor([0], dtype=torch.int32, device=dev)
    mt, nm = m.SearchByProjectionMapPoints(P, fImg, kps, desc, cnt, torch.full((1, cap), -1.0, device=dev),
                                           torch.zeros((1, cap), dtype=torch.uint8, device=dev), nMP, trk,
                                           torch.zeros((1, n), dtype=torch.uint8, device=dev), desc[0:1, :n].contiguous(),
                                           torch.ones((1, n), dtype=torch.uint8, device=dev), 3.0)
    return int(nm[0])


def test_handle_life_cycles_release_their_device_memory():
    import torch
    from morb_slam_amd import ORBextractor, ORBmatcher, Optimizer
    from morb_slam_amd.optimizer import BAProblem, local_bundle_adjustment_fisheye_oneshot, local_bundle_adjustment_oneshot
    big = torch.from_numpy(np.stack([im for s in range(4) for im in make_stereo_pair(1920, 1080, seed=80 + s)])).cuda()   # 4 stereo frames
    small_pairs = [make_stereo_pair(752, 480, seed=90 + s) for s in range(2)]
    small = torch.from_numpy(np.stack([im for p in small_pairs for im in p])).cuda()
    b = make_ba_problem(seed=2, n_free=8, n_fixed=3, n_points=500)
    bf = make_ba_problem_fisheye(seed=1, n_free=6, n_fixed=3, n_points=600)
    ba = (b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    first, after_first = None, None
    for cycle in range(CYCLES):
        ext = ORBextractor(2000, 1.2, 8, 20, 7)
        kb, db, cnt_big, _ = ext.extract_batch(big)
        m = ORBmatcher(0.8, True)
        m.ComputeStereoMatches(ext, kb, db, cnt_big, MBF, MB)
        kps, desc, cnt, _ = ext.extract_batch(small)                      # reconfigure: 752 x 480
        u, _ = m.ComputeStereoMatches(ext, kps, desc, cnt, MBF, MB)
        nproj = _projection_search(m, kps, desc, cnt, ext, u)
        mono, k1, _ = ext(small_pairs[0][0])                               # the single-image host API (pinned staging)
        torch.cuda.synchronize()
        m.close()
        ext.close()

        opt = Optimizer()
        p = BAProblem(opt, *ba)
        p.solve()
        persistent = p.results()
        p.close()
        one = local_bundle_adjustment_oneshot(opt, *ba)
        fish = local_bundle_adjustment_fisheye_oneshot(opt, bf["kfPose"], bf["kfFixed"], bf["mpPos"], bf["eKF"], bf["eMP"], bf["eObs"],
                                                       bf["eRight"], bf["eInvSigma2"], bf["camL"], bf["camR"], bf["Trl"])
        opt.close()
        for x, y in zip(persistent, one):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))

        assert nproj > 0
        got = (cnt_big.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes(), mono, k1.tobytes(), [np.asarray(x).tobytes() for x in persistent],
               [np.asarray(x).tobytes() for x in fish])
        if first is None:
            first = got
            assert len(k1) > 0 and int(cnt_big.min()) > 0
            after_first = _free_bytes()
        else:
            assert got == first, f"cycle {cycle} computed something else than cycle 0"
    after_last = _free_bytes()
    assert after_first - after_last <= BOUND, f"{(after_first - after_last) / 2**20:.1f} MiB less free device memory after {CYCLES} cycles"
