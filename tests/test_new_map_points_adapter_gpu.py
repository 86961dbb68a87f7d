"""ORB_SLAM3::LocalMappingT::CreateNewMapPoints (include/morb/LocalMapping.h), driven from C++ with mock KeyFrame / MapPoint / Atlas
(tests/native/new_map_points_adapter_check.cc) over three neighbours of one keyframe: the created points, the observation tables of
every keyframe (two idx1 sharing one idx2 included: the later AddMapPoint wins on keyframe 2), mlpRecentAddedMapPoints and the atlas
must equal a host replay that runs the CPU oracles neighbour by neighbour; then once more with the second neighbour gated by its
baseline."""
import os
import subprocess

import numpy as np
import pytest

import new_map_points_oracle as oracle
import oracle_lib as O
from morb_slam_amd.capi import KP_DTYPE
from morb_slam_amd.matcher import NEW_MAP_POINT_CREATED
from morb_slam_amd.synth import make_local_mapping_scene, new_map_points_frame_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nmp_adapter") / "new_map_points_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_local_mapping"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", out,
                           os.path.join(NATIVE, "new_map_points_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("gated", [0, 2])
def test_adapter_equals_the_host_replay(exe, tmp_path, gated):
    sc = make_local_mapping_scene(seed=5, B=1, K=3, cap=128, npts=100)
    P = new_map_points_frame_params(sc)
    K, cap, nl = sc["K"], sc["cap"], len(sc["scaleFactors"])
    imgs = [int(sc["img1"][0])] + [int(j) for j in sc["img2"][:, 0]]
    c = sc["cam"]
    cam6 = np.array([c["fx"], c["fy"], c["cx"], c["cy"], sc["mb"], sc["mbf"]], np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K + 1, cap, nl, 0, gated], np.int32).tobytes() + cam6.tobytes() + sc["scaleFactors"].tobytes() + sc["levelSigma2"].tobytes())
        for k, img in enumerate(imgs):
            N = int(sc["count"][img])
            T = (sc["poses"][0, 0, 0:2] if k == 0 else sc["poses"][k - 1, 0, 2:4]).reshape(2, 3, 4)
            ep = np.zeros(2, np.float32) if k == 0 else sc["ep"][k - 1, 0]
            f.write(np.int32(N).tobytes() + np.ascontiguousarray(T[0][:, :3]).tobytes() + np.ascontiguousarray(T[0][:, 3]).tobytes() +
                    np.ascontiguousarray(T[1][:, 3]).tobytes() + ep.astype(np.float32).tobytes() + sc["xy"][img, :N].tobytes() +
                    sc["octave"][img, :N].tobytes() + sc["node"][img, :N].tobytes() + sc["desc"][img, :N].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    first = np.frombuffer(raw[:4 * K], np.int32); off = 4 * K
    nc = int(np.frombuffer(raw[off:off + 4], np.int32)[0]); off += 4
    rec = np.dtype([("kf2", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("status", "<i4"), ("Xw", "<f4", 3), ("normal", "<f4", 3), ("maxD", "<f4"),
                    ("minD", "<f4"), ("desc", "u1", 32)])
    got = np.frombuffer(raw[off:off + nc * rec.itemsize], rec); off += nc * rec.itemsize
    tables = []
    for img in imgs:
        N = int(sc["count"][img])
        tables.append(np.frombuffer(raw[off:off + 4 * N], np.int32)); off += 4 * N
    nr = int(np.frombuffer(raw[off:off + 4], np.int32)[0]); off += 4
    recent = np.frombuffer(raw[off:off + 4 * nr], np.int32); off += 4 * nr
    tail = np.frombuffer(raw[off:off + 12], np.int32)
    assert off + 12 == len(raw)

    # the host replay
    kps = np.zeros((sc["nimg"], cap), KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["octave"] = sc["xy"][..., 0], sc["xy"][..., 1], 31.0, sc["octave"]
    sig, sf, Kc = [float(v) for v in sc["levelSigma2"]], [float(v) for v in sc["scaleFactors"]], [P.fx, P.fy, P.cx, P.cy]
    want = [np.full(int(sc["count"][img]), -1, np.int32) for img in imgs]
    exp = []
    base = dict(npairs=1, nimg=sc["nimg"], cap=cap, count=sc["count"], kps=kps, kpsRaw=None, desc=sc["desc"], uRight=None, depth=None, nLeft1=None,
                nLeft2=None, cam6=cam6, scaleFactors=sc["scaleFactors"], levelSigma2=sc["levelSigma2"], camL8=np.zeros(8, np.float32),
                camR8=np.zeros(8, np.float32), ratioFactor=sc["ratioFactor"], inertial=False, farPoints=False, thFarPoints=0.0)
    i = imgs[0]; ni = int(sc["count"][i])
    shared = 0
    for k in range(K):
        if gated == k + 1:
            continue
        j = imgs[k + 1]; nj = int(sc["count"][j])
        _, me = O.search_for_triangulation(kps[i, :ni], sc["desc"][i, :ni], sc["node"][i, :ni], (want[0] >= 0), None, kps[j, :nj], sc["desc"][j, :nj],
                                           sc["node"][j, :nj], (want[k + 1] >= 0), None, sig, sf, Kc, sc["R12"][k, 0], sc["t12"][k, 0],
                                           sc["ep"][k, 0], False, False, False)
        m12 = np.full((1, cap), -1, np.int32); m12[0, :ni] = me
        o = oracle.run(dict(base, img1=np.array([i], np.int32), img2=np.array([j], np.int32), match12=m12, poses=sc["poses"][k, :1],
                            kf2First=np.array([first[k]], np.uint8)))
        for idx1 in np.nonzero(np.isin(o["status"][0], NEW_MAP_POINT_CREATED))[0]:
            idx2 = int(m12[0, idx1])
            shared += int(want[k + 1][idx2] >= 0)
            want[0][idx1] = want[k + 1][idx2] = len(exp)     # AddMapPoint: the later point takes the neighbour's feature
            t = o["tables"]
            exp.append((k + 1, int(idx1), idx2, int(o["status"][0, idx1]), t["Xw"][0, idx1], t["normal"][0, idx1], t["maxDist"][0, idx1],
                        t["minDist"][0, idx1], t["desc"][0, idx1]))
    assert nc == len(exp) and nc >= (40 if gated else 60), (nc, len(exp))
    assert shared >= 1, "no idx2 shared by two idx1 in the replay"
    for g, e in zip(got, exp):
        assert (g["kf2"], g["idx1"], g["idx2"], g["status"]) == e[:4]
        assert np.abs(g["Xw"] - e[4]).max() <= 1e-4 * max(1.0, np.abs(e[4]).max()) and np.abs(g["normal"] - e[5]).max() <= 1e-4
        assert abs(g["maxD"] - e[6]) <= 1e-4 * max(1.0, e[6]) and abs(g["minD"] - e[7]) <= 1e-4 * max(1.0, e[7])
        assert np.array_equal(g["desc"], e[8])
    for k in range(K + 1):
        assert np.array_equal(tables[k], want[k]), k
    if gated:
        assert (tables[gated] == -1).all()
    assert np.array_equal(recent, np.arange(nc))
    assert tail.tolist() == [nc, 0, 0]    # the atlas holds the points in order; observations agree; every point updated exactly once
