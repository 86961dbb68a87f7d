"""The case of the TrackLocalMapChain test: a make_local_map_scene map whose points are the extracted ORB features of two synthetic
images, back-projected to random depths from the identity pose, so that isInFrustum, SearchByProjection(F, MapPoints) and
PoseOptimization have real work; and the run it is compared with: the EXISTING kernels fed with the oracle's local map, gathered on
the host into the per-frame tables they have always taken."""
import ctypes as C

import numpy as np

import local_map_oracle as oracle

W, H, FX, FY, CX, CY = 640, 480, 458.654, 457.296, 320.0, 240.0
MP_CAP, KF_OUT, TH = 2048, 64, 3.0


def chain_case(dev, B=3):
    import torch
    from morb_slam_amd import ORBextractor, ORBmatcher
    from morb_slam_amd.capi import KP_DTYPE, make_frame_params
    from morb_slam_amd.synth import make_image, make_local_map_scene
    from morb_slam_amd.tracking import TrackLocalMapChain
    rng = np.random.default_rng(77)
    imgs = np.stack([make_image(W, H, seed=31 + i) for i in range(2)])
    ext = ORBextractor(800, 1.2, 8, 20, 7, device=0)
    kps, desc, cnt, _ = ext.extract_batch(torch.from_numpy(imgs).to(dev))
    torch.cuda.synchronize()
    cap = kps.shape[1]
    kh = kps.cpu().numpy().reshape(2, cap, 28).view(KP_DTYPE).reshape(2, cap)
    dh, ch = desc.cpu().numpy(), cnt.cpu().numpy()
    P = make_frame_params(W, H, FX, FY, CX, CY, 0.0, 0.0, ext.GetScaleFactors(), ext.GetScaleSigmaSquares())
    cam = dict(fx=FX, fy=FY, cx=CX, cy=CY, bf=0.0)
    sf = np.array(list(P.scaleFactors)[:P.nlevels], np.float32)
    first = np.array([0, int(ch[0])])                     # map rows of image 0's features, then image 1's
    nmp = int(ch[0] + ch[1])
    scene = make_local_map_scene(seed=9, nkf=40, nmp=nmp, kf_cap=384, nq=B, track=6)
    for img in range(2):
        n = int(ch[img])
        k = kh[img, :n]
        z = rng.uniform(2.0, 8.0, n).astype(np.float32)
        X = np.stack([(k["x"] - np.float32(CX)) * z / np.float32(FX), (k["y"] - np.float32(CY)) * z / np.float32(FY), z], 1).astype(np.float32)
        dist = np.linalg.norm(X, axis=1).astype(np.float32)
        nrm = X / dist[:, None] + rng.normal(0, 0.1, X.shape)
        rows = slice(first[img], first[img] + n)
        scene["mpPw"][rows] = X
        scene["mpNormal"][rows] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        maxD = (dist * sf[k["octave"]] * rng.uniform(1.0, 1.2, n)).astype(np.float32)
        scene["mpMaxD"][rows], scene["mpMinD"][rows] = maxD, (maxD / sf[P.nlevels - 1]).astype(np.float32)
        scene["mpDesc"][rows] = dh[img, :n]
    # the frames: frame q shows image q % 2 from keyframe c's place and holds 70 % of that image's points that keyframes c, c + 1 hold
    curImg = np.arange(B, dtype=np.int32) % 2
    frameMp, pose0 = np.full((B, cap), -1, np.int32), np.zeros((B, 7), np.float32)
    for q in range(B):
        c = int(scene["lastKf"][q])
        held = np.unique(np.concatenate([scene["kfMp"][k, :scene["kfCount"][k]] for k in (c, c + 1)]))
        img = int(curImg[q])
        feat = held[(held >= first[img]) & (held < first[img] + ch[img])] - first[img]
        feat = feat[rng.random(len(feat)) < 0.7]
        frameMp[q, feat] = feat + first[img]
        rv = rng.normal(0, 0.001, 3)
        quat = np.concatenate([rv / 2, [1.0]])
        pose0[q] = np.concatenate([quat / np.linalg.norm(quat), rng.normal(0, 0.005, 3)]).astype(np.float32)
    scene = dict(scene, frameMp=frameMp, count=ch[curImg].astype(np.int32), cap=cap)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tables = ORBmatcher.local_map_tables(scene, dev)
    chain = TrackLocalMapChain(P, cam, kps, desc, cnt, None, tables, t(curImg), t(frameMp), t(pose0), t(scene["lastKf"].astype(np.int32)),
                               inertial=False, kf_out=KF_OUT, mp_cap=MP_CAP, th_local=TH, device=0)
    chain._keep = ext
    return dict(chain=chain, scene=scene, P=P, cam=cam, kps=kps, desc=desc, cnt=cnt, curImg=t(curImg), pose0=t(pose0), cap=cap)


def reference_run(case, dev):
    """The oracle's local map, gathered on the host, through the kernels TrackingChain runs for TrackLocalMap."""
    import torch
    from morb_slam_amd import ORBmatcher, Optimizer
    from morb_slam_amd.capi import check, lib, ptr
    s, P, cap = case["scene"], case["P"], case["cap"]
    e = oracle.expected(s, False, kf_out=KF_OUT, mp_cap=MP_CAP)
    assert not e["overflow"].any()
    B = len(s["count"])
    tab = dict(Pw=np.zeros((B, MP_CAP, 3), np.float32), normal=np.zeros((B, MP_CAP, 3), np.float32), maxDist=np.zeros((B, MP_CAP), np.float32),
               minDist=np.zeros((B, MP_CAP), np.float32), mpDesc=np.zeros((B, MP_CAP, 32), np.uint8), mpHasObs=np.zeros((B, MP_CAP), np.uint8))
    src = dict(Pw="mpPw", normal="mpNormal", maxDist="mpMaxD", minDist="mpMinD", mpDesc="mpDesc", mpHasObs="mpObserved")
    for q in range(B):
        rows = e["full"][q]["localMp"]
        for k, v in src.items():
            tab[k][q, :len(rows)] = s[v][rows]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    G = {k: t(v) for k, v in tab.items()}
    nMP, frameMP, pose = t(e["nLocalMp"]), t(e["frameLocal"]), case["pose0"].clone()
    m, opt, L = ORBmatcher(0.8, True), Optimizer(), lib()
    try:
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        blocked, mpSeen, noOut = z((B, cap), u8), z((B, MP_CAP), u8), z((B, cap), u8)
        nm1, nmMap1, nInl, nInlMap = z((B,), i32), z((B,), i32), z((B,), i32), z((B,), i32)
        Rcw, tcw, Ow = z((B, 9), f32), z((B, 3), f32), z((B, 3), f32)
        hasMP, obs, invS2, Xw = z((B, cap), u8), z((B, cap, 3), f32), z((B, cap), f32), z((B, cap, 3), f32)
        cur, kps, desc, cnt = case["curImg"], case["kps"], case["desc"], case["cnt"]
        trk = dict(inView=z((B, MP_CAP), u8), projX=z((B, MP_CAP), f32), projY=z((B, MP_CAP), f32), projXR=z((B, MP_CAP), f32),
                   depth=z((B, MP_CAP), f32), level=z((B, MP_CAP), i32), viewCos=z((B, MP_CAP), f32))
        nmLocal, po = z((B,), i32), (z((B,), i32), z((B, cap), u8), z((B, 2), i32))
        # one explicit stream for both handles: each handle's own stream is ordered with the default stream only, not with the other's
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        st, sp = stream.cuda_stream, C.c_void_p(stream.cuda_stream)
        check(L.morb_track_discard_outliers_batch(m._h, B, ptr(cur), cap, ptr(cnt), ptr(frameMP), ptr(noOut), MP_CAP, ptr(G["mpHasObs"]), ptr(blocked),
                                                  ptr(mpSeen), ptr(nm1), ptr(nmMap1), sp))
        check(L.morb_frame_set_pose_batch(m._h, B, ptr(pose), ptr(Rcw), ptr(tcw), ptr(Ow), sp))
        m.isInFrustum(P, Rcw, tcw, Ow, nMP, G["Pw"], G["normal"], G["maxDist"], G["minDist"], 0.5, out=trk, stream=st)
        m.SearchByProjectionMapPoints(P, cur, kps, desc, cnt, None, blocked, nMP, trk, mpSeen, G["mpDesc"], G["mpHasObs"], TH, False, 0.0,
                                      matchF=frameMP, nm=nmLocal, stream=st)
        check(L.morb_pose_edges_batch(m._h, C.byref(P), B, ptr(cur), cap, ptr(cnt), ptr(kps), None, None, None, 0, MP_CAP, ptr(G["Pw"]), ptr(frameMP),
                                      ptr(hasMP), ptr(obs), ptr(invS2), ptr(Xw), sp))
        opt.PoseOptimization(hasMP, obs, invS2, Xw, pose, case["cam"], out=po, stream=st)
        check(L.morb_track_discard_outliers_batch(m._h, B, ptr(cur), cap, ptr(cnt), ptr(frameMP), ptr(po[1]), MP_CAP, ptr(G["mpHasObs"]), None, None,
                                                  ptr(nInl), ptr(nInlMap), sp))
        torch.cuda.synchronize()
        return dict(frameMP=frameMP.cpu().numpy(), pose=pose.cpu().numpy(), nLocalMp=e["nLocalMp"], nmLocal=nmLocal.cpu().numpy(), nInl=nInl.cpu().numpy())
    finally:
        m.close()
        opt.close()
