"""Scenes the projection-search tests share (test_matcher_gpu.py, test_search_tiers_gpu.py): synthetic stereo frames extracted on the GPU
(bit-exact with the oracle), their stereo matches, and the map points and keyframes built from them.  Plain helpers, not fixtures: each
test module caches what it builds."""
import os

import numpy as np

import oracle_lib as O

# (fx, fy, cx, cy, baseline) per image size: EuRoC, KITTI (00-02 calibration), a 1080p camera
CAMERAS = {(752, 480): (458.654, 457.296, 367.215, 248.375, 0.11),
           (1241, 376): (718.856, 718.856, 607.1928, 185.2157, 0.537150588),
           (1920, 1080): (1400.0, 1400.0, 960.0, 540.0, 0.12)}


def make_batch(width=752, height=480, nfeatures=1200, npairs=2, seed=60):
    """2 * npairs stereo frames (npairs pairs, then a shifted copy of each), extracted on the GPU and checked bit-exact with the oracle.
    Images 2f / 2f + 1 are frame f's left / right; frame npairs + i is a shifted copy of frame i."""
    import torch
    from morb_slam_amd import KP_DTYPE, ORBextractor
    from morb_slam_amd.synth import make_stereo_pair, shift_image
    off = 10 * int(os.environ.get("MORB_TEST_SEED", "0"))   # (tools/stress_matchers.sh: the whole file again on other images)
    pairs = [make_stereo_pair(width, height, seed=seed + off + i) for i in range(npairs)]
    shifts = [(4, 2), (7, -3)]
    pairs += [tuple(shift_image(im, *shifts[i % 2]) for im in pairs[i]) for i in range(npairs)]
    imgs = np.stack([im for p in pairs for im in p])
    ext = ORBextractor(nfeatures, 1.2, 8, 20, 7)
    d = torch.from_numpy(imgs).cuda()
    kps, desc, cnt, mono = ext.extract_batch(d)
    torch.cuda.synchronize()
    ora = []
    for im in imgs:
        o = O.OracleExtractor(nfeatures)
        _, k, dd = o(im)
        ora.append((o, k, dd))
    c = cnt.cpu().numpy()
    for i in range(len(imgs)):
        assert kps[i, :c[i]].cpu().numpy().reshape(-1).view(KP_DTYPE).tobytes() == ora[i][1].tobytes()
    fx, fy, cx, cy, b = CAMERAS[(width, height)]
    return dict(ext=ext, kps=kps, desc=desc, cnt=cnt, ora=ora, imgs=imgs, KP=KP_DTYPE, size=(width, height),
                cam=(fx, fy, cx, cy, float(np.float32(fx * b)), float(np.float32(b))), npairs=npairs)


def scene(batch):
    """Frame parameters of the batch's camera and the stereo matches (uRight, depth) of every frame: [nframes, cap] device tensors."""
    import torch
    from morb_slam_amd import ORBmatcher
    from morb_slam_amd.capi import make_frame_params
    ext = batch["ext"]
    fx, fy, cx, cy, mbf, mb = batch["cam"]
    P = make_frame_params(*batch["size"], fx, fy, cx, cy, mbf, mb, ext.GetScaleFactors(), ext.GetScaleSigmaSquares())
    m = ORBmatcher(0.8, True)
    u, d = m.ComputeStereoMatches(ext, batch["kps"], batch["desc"], batch["cnt"], np.float32(mbf), np.float32(mb))
    torch.cuda.synchronize()
    return P, u, d


def quat_from_R(R):
    from morb_slam_amd.synth import _quat_from_R as q
    return q(R)


def lc_scene(batch, shifted=None):
    """Keyframe A = image 0 (world = its camera frame), keyframe B = the left image of frame 0's shifted copy with a nearby pose;
    map points = stereo back-projections of each keyframe's own features.  Keys of the result: the two image indices."""
    from morb_slam_amd.synth import _quat_from_rotvec, _quat_rot
    P, uR, dep = scene(batch)
    rng = np.random.default_rng(21)
    out = {}
    fB = batch.get("npairs", 2) if shifted is None else shifted
    q2 = _quat_from_rotvec(np.array([0.002, -0.004, 0.001])); t2 = np.array([-0.03, -0.015, 0.01])
    T = {0: np.array([0, 0, 0, 1, 0, 0, 0], np.float64), 2 * fB: np.concatenate([q2, t2])}
    for img, fr in ((0, 0), (2 * fB, fB)):
        k, d = batch["ora"][img][1], batch["ora"][img][2]
        z = dep[fr, :len(k)].cpu().numpy()
        Xc = np.stack([(k["x"] - P.cx) * np.abs(z) / P.fx, (k["y"] - P.cy) * np.abs(z) / P.fy, np.abs(z)], 1)
        qinv = T[img][:4] * np.array([-1, -1, -1, 1])
        Xw = np.array([_quat_rot(qinv, x - T[img][4:]) for x in Xc]).reshape(-1, 3)
        dist = np.linalg.norm(Xc, axis=1)
        maxD = dist * 1.2 ** k["octave"] * rng.uniform(0.9, 1.3, len(k)); minD = maxD / 1.2 ** 7
        Ow = -_quat_rot(qinv, T[img][4:])
        nrm = (Xw - Ow) / np.linalg.norm(Xw - Ow, axis=1, keepdims=True) + rng.normal(0, 0.2, Xw.shape)
        out[img] = dict(k=k, d=d, valid=z > 0, Xw=Xw.astype(np.float32), maxD=maxD.astype(np.float32), minD=minD.astype(np.float32),
                        normal=nrm.astype(np.float32), T=T[img].astype(np.float32), Ow=Ow.astype(np.float32),
                        uR=uR[fr, :len(k)].cpu().numpy())
    return P, out
