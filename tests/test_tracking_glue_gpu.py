"""The three marshalling kernels of csrc/tracking.hip alone, on constructed tables, bit for bit against the oracle (oracle_lib.frame_set_pose, pose_edges,
discard_outliers).  Inside the tracking chain they only ever see one capacity, in-range remap entries and map-point indices, and one fixed set of
nullable arguments; here: 65 frames for the 64-thread k_set_pose, capacities either side of k_pose_edges' 256-thread blocks and of k_discard's 1024-thread
trips, indices at and beyond their tables' ends, every nullable argument NULL in turn, a frame index that differs from its image index, an empty frame,
and sentinels past each frame's count."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import projection_cases as PC

pytestmark = pytest.mark.gpu
SENT = -7777


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _matcher():
    from morb_slam_amd import ORBmatcher
    return ORBmatcher(0.8, True)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_frame_set_pose():
    import torch
    from morb_slam_amd.capi import check, ptr
    rng = np.random.default_rng(5)
    nxt = lambda v, n: PC.up(v, n) if n > 0 else PC.dn(v, -n)
    poses = [[0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, 2, 3], [0, 1, 0, 0, -1, 2, -3], [0, 0, 1, 0, 0.5, 0.25, -8],     # identity, 180 degrees about x, y, z
             [0, 0, 0, -1, 1, 1, 1], [-0.5, 0.5, -0.5, -0.5, 3, -4, 5],                                             # w < 0
             [0, 0, 0, nxt(1.0, 3), 1, 2, 3], [0.5, 0.5, 0.5, nxt(0.5, -4), -7, 8, 9], [nxt(0.6, 2), 0, nxt(0.8, -3), 0, 1, 0, 0],   # a few ulp off unit length
             [0.6, 0, 0, 0.8, 1e6, -2.5e6, 7.75e6], [0, -0.28, 0.96, 0, -1e7, 3e-7, 1e7]]                              # large translations
    while len(poses) < 65:
        q = rng.normal(size=4); q = (q / np.linalg.norm(q)).astype(np.float32)
        poses.append(list(q) + list(rng.uniform(-50, 50, 3) * (1000 if len(poses) % 7 == 0 else 1)))
    pose = np.array(poses, np.float32)
    assert pose.shape == (65, 7) and (pose[:, 3] < 0).sum() >= 2
    F = len(pose)
    m = _matcher()
    R = torch.full((F + 1, 9), float(SENT), device="cuda"); t = torch.full((F + 1, 3), float(SENT), device="cuda"); Ow = torch.full((F + 1, 3), float(SENT), device="cuda")
    d_pose = _cu(pose)        # (every device tensor keeps a name until the synchronize: a temporary's block goes back to the allocator at once)
    check(m._L.morb_frame_set_pose_batch(m._h, F, ptr(d_pose), ptr(R), ptr(t), ptr(Ow), None))
    torch.cuda.synchronize()
    R, t, Ow = R.cpu().numpy(), t.cpu().numpy(), Ow.cpu().numpy()
    for f in range(F):
        eR, et, eO = O.frame_set_pose(pose[f])
        _bits(R[f], eR, ("Rcw", f)); _bits(t[f], et, ("tcw", f)); _bits(Ow[f], eO, ("Ow", f))
    assert (R[F] == SENT).all() and (t[F] == SENT).all() and (Ow[F] == SENT).all()      # nothing written past frame 64
    assert np.array_equal(R[0], np.eye(3, dtype=np.float32).reshape(9)) and np.array_equal(R[1], np.diag([1, -1, -1]).astype(np.float32).reshape(9))


def _frames(cap, rng, counts):
    """Images with the given feature counts: keypoints with octaves 0 .. 7 (0 and 7 at the ends), and the frame -> image map reversed."""
    nimg = len(counts)
    k = np.zeros((nimg, cap), O.KP_DTYPE)
    k["x"] = rng.uniform(0, 512, (nimg, cap)).astype(np.float32); k["y"] = rng.uniform(0, 384, (nimg, cap)).astype(np.float32)
    k["octave"] = rng.integers(0, 8, (nimg, cap)); k["octave"][:, 0] = 0; k["octave"][:, 1] = 7
    fImg = np.arange(nimg, dtype=np.int32)[::-1].copy()
    assert (fImg != np.arange(nimg)).any()
    return k, np.array(counts, np.int32), fImg


@pytest.mark.parametrize("cap", [255, 256, 257])
@pytest.mark.parametrize("mode", ["frameMP", "match", "match_remap"])
@pytest.mark.parametrize("stereo", [False, True])
def test_pose_edges(cap, mode, stereo):
    import torch
    from morb_slam_amd.capi import check, ptr
    rng = np.random.default_rng(cap * 7 + len(mode))
    mpCap, remapCap = 61, 50
    k, count, fImg = _frames(cap, rng, [cap, 0, 100, 1])
    F = len(fImg)
    P = PC.params("p12")
    uR = np.where(rng.random((F, cap)) < 0.5, rng.uniform(1, 500, (F, cap)), -1.0).astype(np.float32)
    mpXw = rng.normal(size=(F, mpCap, 3)).astype(np.float32)
    # the table the kernel reads: every kind of value in the first rows of every frame, random beyond
    top = remapCap if mode == "match_remap" else mpCap
    src = rng.integers(-1, top + 3, (F, cap)).astype(np.int32)
    src[:, :6] = [-1, 0, top - 1, top, top + 1, 2 ** 30]
    remap = rng.integers(-1, mpCap + 2, (F, remapCap)).astype(np.int32)
    remap[:, :4] = [mpCap - 1, mpCap, -1, 0]; remap[:, remapCap - 1] = mpCap - 1
    src[:, 6:10] = [0, 1, 2, 3] if mode == "match_remap" else src[:, 6:10]
    # the resolved map point per feature, by the header's rules: match -> remap (a match at or beyond remapCap is -1) -> an index at or beyond mpCap is -1
    want = np.full((F, cap), -1, np.int32)
    for f in range(F):
        for j in range(count[fImg[f]]):
            mp = int(src[f, j])
            if mode == "match_remap" and mp >= 0:
                mp = int(remap[f, mp]) if mp < remapCap else -1
            want[f, j] = mp if mp < mpCap else -1
    assert (want == mpCap - 1).any() and ((src >= top) & (np.arange(cap)[None] < count[fImg][:, None])).any()
    frameMP = src.copy() if mode == "frameMP" else np.full((F, cap), SENT, np.int32)
    d_frameMP = _cu(frameMP)
    hasMP = torch.full((F, cap), 9, dtype=torch.uint8, device="cuda"); obs = torch.full((F, cap, 3), float(SENT), device="cuda")
    is2 = torch.full((F, cap), float(SENT), device="cuda"); Xw = torch.full((F, cap, 3), float(SENT), device="cuda")
    m = _matcher()
    d_match = None if mode == "frameMP" else _cu(src)
    d_remap = _cu(remap) if mode == "match_remap" else None
    d_uR = _cu(uR) if stereo else None
    kps = _cu(k.view(np.uint8).reshape(len(count), cap, 28))
    d_fImg, d_count, d_mpXw = _cu(fImg), _cu(count), _cu(mpXw)     # named: alive until the synchronize below
    check(m._L.morb_pose_edges_batch(m._h, C.byref(P), F, ptr(d_fImg), cap, ptr(d_count), ptr(kps), ptr(d_uR), ptr(d_match), ptr(d_remap),
                                     remapCap if mode == "match_remap" else 0, mpCap, ptr(d_mpXw), ptr(d_frameMP), ptr(hasMP), ptr(obs), ptr(is2), ptr(Xw), None))
    torch.cuda.synchronize()
    hasMP, obs, is2, Xw, gotMP = hasMP.cpu().numpy(), obs.cpu().numpy(), is2.cpu().numpy(), Xw.cpu().numpy(), d_frameMP.cpu().numpy()
    invS = (np.float32(1.0) / PC.sigma2("p12")).astype(np.float32)
    for f in range(F):
        n = int(count[fImg[f]])
        Fo = O.make_frame(P, k[fImg[f], :n], np.zeros((n, 32), np.uint8), uR[f, :n] if stereo else None)
        eh, eo, es, eX = O.pose_edges(Fo, invS, want[f, :n], mpXw[f])
        _bits(hasMP[f, :n], eh, ("hasMP", f)); _bits(obs[f, :n], eo, ("obs", f)); _bits(is2[f, :n], es, ("invSigma2", f)); _bits(Xw[f, :n], eX, ("Xw", f))
        # rows at or beyond the count: no edge
        assert (hasMP[f, n:] == 0).all() and (obs[f, n:] == np.array([0, 0, -1], np.float32)).all() and (is2[f, n:] == 0).all() and (Xw[f, n:] == 0).all()
        if mode == "frameMP":
            _bits(gotMP[f], frameMP[f], ("frameMP is only read", f))
        else:
            _bits(gotMP[f, :n], want[f, :n], ("frameMP", f))
            assert (gotMP[f, n:] == -1).all()
    if not stereo:
        assert (obs[:, :, 2] == -1).all()


@pytest.mark.parametrize("cap,mpCap", [(100, 100), (1025, 2049), (2049, 1025), (100, 2049), (2049, 100)])
@pytest.mark.parametrize("null", ["none", "mpHasObs", "blocked", "mpSeen", "nmatches", "nmatchesMap"])
def test_discard_outliers(cap, mpCap, null):
    import torch
    from morb_slam_amd.capi import check, ptr
    rng = np.random.default_rng(cap * 31 + mpCap + len(null))
    k, count, fImg = _frames(cap, rng, [cap, 0, cap // 2, 1])
    F = len(fImg)
    frameMP = np.where(rng.random((F, cap)) < 0.6, rng.integers(0, mpCap, (F, cap)), -1).astype(np.int32)
    frameMP[:, :4] = [mpCap - 1, 0, mpCap - 1, -1]                 # two features hold the same point, the last row of the point table among them
    outlier = (rng.random((F, cap)) < 0.3).astype(np.uint8)
    outlier[:, :4] = [1, 0, 0, 1]                                 # one of the two holders is an outlier: cleared, its point still seen; an outlier without a point
    hasObs = (rng.random((F, mpCap)) < 0.7).astype(np.uint8)
    for f in range(F):                                            # sentinels past the count
        n = int(count[fImg[f]])
        frameMP[f, n:] = SENT; outlier[f, n:] = 9
    d_fm, d_ol = _cu(frameMP), _cu(outlier)
    blocked = torch.full((F, cap), 9, dtype=torch.uint8, device="cuda"); seen = torch.full((F, mpCap), 9, dtype=torch.uint8, device="cuda")
    nm = torch.full((F,), SENT, dtype=torch.int32, device="cuda"); nmap = torch.full((F,), SENT, dtype=torch.int32, device="cuda")
    m = _matcher()
    arg = lambda name, t: None if null == name else ptr(t)
    d_fImg, d_count, d_hasObs = _cu(fImg), _cu(count), _cu(hasObs)     # named: alive until the synchronize below
    check(m._L.morb_track_discard_outliers_batch(m._h, F, ptr(d_fImg), cap, ptr(d_count), ptr(d_fm), ptr(d_ol), mpCap, arg("mpHasObs", d_hasObs),
                                                 arg("blocked", blocked), arg("mpSeen", seen), arg("nmatches", nm), arg("nmatchesMap", nmap), None))
    torch.cuda.synchronize()
    g_fm, g_ol, g_blk, g_seen, g_nm, g_nmap = [x.cpu().numpy() for x in (d_fm, d_ol, blocked, seen, nm, nmap)]
    for f in range(F):
        n = int(count[fImg[f]])
        ho = np.ones(mpCap, np.uint8) if null == "mpHasObs" else hasObs[f]        # NULL counts every point as observed
        e_nm, e_nmap, e_fm, e_blk, e_seen = O.discard_outliers(frameMP[f, :n], outlier[f, :n], ho)
        _bits(g_fm[f, :n], e_fm, ("frameMP", f))
        # mvbOutlier is cleared inside `if (pMP)` (Tracking.cc:2716-2740): a flag on a feature without a map point stays
        _bits(g_ol[f, :n], np.where(frameMP[f, :n] >= 0, 0, outlier[f, :n]).astype(np.uint8), ("outlier", f))
        assert (g_fm[f, n:] == SENT).all() and (g_ol[f, n:] == 9).all()                     # rows past the count keep their sentinels
        if null != "blocked":
            _bits(g_blk[f, :n], e_blk, ("blocked", f)); assert (g_blk[f, n:] == 0).all()   # (blocked IS written there, as 0)
        else:
            assert (g_blk == 9).all()
        if null != "mpSeen":
            _bits(g_seen[f], e_seen, ("mpSeen", f))
        else:
            assert (g_seen == 9).all()
        assert g_nm[f] == (SENT if null == "nmatches" else e_nm) and g_nmap[f] == (SENT if null == "nmatchesMap" else e_nmap), (f, g_nm[f], e_nm, g_nmap[f], e_nmap)
        if n >= 4:
            assert g_fm[f, 0] == -1 and g_fm[f, 2] == mpCap - 1 and (null == "mpSeen" or g_seen[f, mpCap - 1] == 1)
