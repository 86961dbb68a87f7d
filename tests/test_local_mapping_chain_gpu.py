"""tracking.LocalMappingChain: search, create and Fuse over K neighbour ranks of B new keyframes on one stream, against a host replay that
runs each stage's CPU oracle in the reference's order (rank by rank, hasMP carried along), on synth.make_local_mapping_scene."""
import numpy as np
import pytest
import torch

import new_map_points_oracle as oracle
import oracle_lib as O
from morb_slam_amd.capi import KP_DTYPE
from morb_slam_amd.matcher import NEW_MAP_POINT_CREATED
from morb_slam_amd.synth import make_local_mapping_scene, new_map_points_frame_params
from morb_slam_amd.tracking import LocalMappingChain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_chain_equals_the_host_replay():
    sc = make_local_mapping_scene(seed=2, B=2, K=3, cap=128, npts=100)
    P = new_map_points_frame_params(sc)
    nimg, cap, B, K = sc["nimg"], sc["cap"], sc["B"], sc["K"]
    kps = np.zeros((nimg, cap), KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["octave"] = sc["xy"][..., 0], sc["xy"][..., 1], 31.0, sc["octave"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    chain = LocalMappingChain(P, t(kps.view(np.uint8).reshape(nimg, cap, 28)), t(sc["desc"]), t(sc["node"]), t(sc["count"]), sc)
    try:
        chain.step()
        chain.sync()
        g_tables = {k: v.cpu().numpy() for k, v in chain.tables.items()}
        g_has = chain.hasMP.cpu().numpy()
        g_tri = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in chain.tri]
        g_created = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in chain.created]
        g_fused = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in chain.fused]
        g_valid = [v.cpu().numpy() for v in chain.valid]
    finally:
        chain.close()
    # the host replay
    sig, sf, Kc = [float(v) for v in sc["levelSigma2"]], [float(v) for v in sc["scaleFactors"]], [P.fx, P.fy, P.cx, P.cy]
    has = np.zeros((nimg, cap), np.uint8)
    tables = oracle.empty_tables(B, cap)
    c = sc["cam"]
    base = dict(npairs=B, nimg=nimg, cap=cap, img1=sc["img1"], count=sc["count"], kps=kps, kpsRaw=None, desc=sc["desc"], uRight=None, depth=None,
                nLeft1=None, nLeft2=None, cam6=np.array([c["fx"], c["fy"], c["cx"], c["cy"], sc["mb"], sc["mbf"]], np.float32),
                scaleFactors=sc["scaleFactors"], levelSigma2=sc["levelSigma2"], camL8=np.zeros(8, np.float32), camR8=np.zeros(8, np.float32),
                ratioFactor=sc["ratioFactor"], inertial=False, farPoints=False, thFarPoints=0.0)
    total = 0
    for k in range(K):
        m12 = np.full((B, cap), -1, np.int32)
        for b in range(B):
            i, j = sc["img1"][b], sc["img2"][k, b]
            ni, nj = sc["count"][i], sc["count"][j]
            r, me = O.search_for_triangulation(kps[i, :ni], sc["desc"][i, :ni], sc["node"][i, :ni], has[i, :ni], None, kps[j, :nj],
                                               sc["desc"][j, :nj], sc["node"][j, :nj], has[j, :nj], None, sig, sf, Kc, sc["R12"][k, b],
                                               sc["t12"][k, b], sc["ep"][k, b], False, False, False)
            m12[b, :ni] = me
            assert int(g_tri[k][1][b]) == r and np.array_equal(g_tri[k][0][b, :ni], me), (k, b)
        before = has[sc["img1"]].copy()
        o = oracle.run(dict(base, img2=sc["img2"][k], match12=m12, poses=sc["poses"][k], kf2First=sc["kf2First"][k]), tables=tables, hasMP=has)
        assert np.array_equal(g_created[k][0], o["status"]) and np.array_equal(g_created[k][1], o["stats"]), k
        made = np.isin(o["status"], NEW_MAP_POINT_CREATED)
        assert not (made & (before > 0)).any()        # a later rank creates nothing at a feature that has a point
        total += int(made.sum())
        if k > 0:
            assert made.sum() > 0 and (before > 0).sum() > 0
    assert total >= 100 and np.array_equal(g_has, has)
    for n in ("desc", "img2", "idx2"):
        assert np.array_equal(g_tables[n], tables[n]), n
    got = g_tables["img2"] >= 0
    for n in ("Xw", "normal", "maxDist", "minDist"):
        assert np.abs(g_tables[n][got] - tables[n][got]).max() <= 1e-4 * max(1.0, np.abs(tables[n][got]).max()), n
    assert len(np.unique(g_tables["img2"][got])) == B * K     # every rank contributed
    # Fuse: into neighbour k goes every new point but those created with it
    invS = (1.0 / sc["levelSigma2"]).astype(np.float32)
    nfound = 0
    for k in range(K):
        for b in range(B):
            j = sc["img2"][k, b]; nj = sc["count"][j]
            valid = (g_tables["img2"][b] >= 0) & (g_tables["img2"][b] != j)
            assert np.array_equal(g_valid[k][b] != 0, valid) and valid.any() and (g_tables["img2"][b] == j).any()
            Fo = O.make_frame(P, kps[j, :nj], sc["desc"][j, :nj], None)
            ei, ed = O.fuse_search(Fo, invS, sc["Tcw7"][k, b], sc["Ow"][k, b], valid, g_tables["Xw"][b], g_tables["normal"][b],
                                   g_tables["maxDist"][b], g_tables["minDist"][b], g_tables["desc"][b], 3.0, False)
            assert np.array_equal(g_fused[k][0][b], ei) and np.array_equal(g_fused[k][1][b], ed), (k, b)
            nfound += int((ei >= 0).sum())
    assert nfound > 0   # points made with one neighbour are found in another that sees them
