"""LocalMapping::CreateNewMapPoints without a GPU: the shared header include/morb/new_map_points_math.h through the CPU oracle
(tests/native/new_map_points_oracle.cc) on the corpus of tests/new_map_points_corpus.py, the header alone in a program built with the
host sanitizers, and the surfaces the feature adds (exports, Python front, scene generator)."""
import os
import re
import subprocess

import numpy as np

import new_map_points_corpus as corpus
import new_map_points_oracle as oracle
from morb_slam_amd.matcher import NEW_MAP_POINT_CREATED, NEW_MAP_POINT_STATS, NEW_MAP_POINT_STATUS
from morb_slam_amd.synth import NEW_MAP_POINT_CATEGORIES, NEW_MAP_POINT_KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
ST = {n: k for k, n in enumerate(NEW_MAP_POINT_STATUS)}
NOISY = [NEW_MAP_POINT_CATEGORIES.index(c) for c in ("reproj1", "reproj2", "stereo_noisy")]


def test_enums_of_the_header_are_the_python_tuples():
    status, stats = oracle.names()
    assert status == NEW_MAP_POINT_STATUS and stats == NEW_MAP_POINT_STATS
    assert NEW_MAP_POINT_CREATED == (ST["TRIANGULATED"], ST["STEREO1"], ST["STEREO2"])


def test_corpus_shape():
    sc = corpus.scenes()
    assert [s["kind"] for s in sc] == list(NEW_MAP_POINT_KINDS) and sum(s["npairs"] for s in sc) == 16
    for s in sc:
        assert s["cap"] == 96 and s["count"].min() >= 40 and s["count"].max() <= 96
        for p in range(s["npairs"]):
            m = s["match12"][p]
            assert m.max() < s["count"][s["img2"][p]] and (m[s["count"][s["img1"][p]]:] == -1).all()
            assert (np.bincount(m[m >= 0]) > 1).sum() >= 1, "no idx2 shared by two idx1"
        assert set(np.unique(s["img1"])).isdisjoint(np.unique(s["img2"])) and len(np.unique(s["img1"])) == s["npairs"]
    assert sc[1]["uRight"][sc[1]["img1"]].max() >= 0 and sc[1]["uRight"][sc[1]["img2"]].max() < 0
    assert sc[2]["uRight"][sc[2]["img2"]].max() >= 0 and sc[2]["uRight"][sc[2]["img1"]].max() < 0
    assert (sc[3]["nLeft"] > 0).all() and (sc[3]["nLeft"] < sc[3]["count"]).all()


def test_every_status_occurs_in_the_corpus_but_the_two_exact_zeros():
    h = corpus.status_histogram()
    print({n: int(h[k]) for k, n in enumerate(NEW_MAP_POINT_STATUS)})
    for n, k in ST.items():
        if n in ("NONE", "TRIANGULATE_FALSE", "ZERO_DIST"):
            assert h[k] == 0, n
        else:
            assert h[k] > 0, n
    # the 0.9996 of the inertial form and the 0.9998 of the other both decide; each kind creates points; the rig uses all four side pairs
    for s, r in zip(corpus.scenes(), corpus.results()):
        assert (r["stats"][:, 0] > 0).all(), s["kind"]
        assert ((r["status"] == ST["NONE"]) == (s["match12"] < 0)).all()
    s, r = corpus.scenes()[3], corpus.results()[3]
    sides = set()
    for p in range(s["npairs"]):
        i1 = np.nonzero(np.isin(r["status"][p], NEW_MAP_POINT_CREATED))[0]
        sides |= set(zip((i1 >= s["nLeft"][s["img1"][p]]).tolist(), (s["match12"][p][i1] >= s["nLeft"][s["img2"][p]]).tolist()))
    assert len(sides) == 4


def test_the_two_exact_zeros_by_hand():
    """x3Dh(3) == 0 needs parallel rays, which the parallax test turns away first, and dist == 0 needs the point at a camera centre, where
    z <= 0 comes first: only inputs that no pair of keyframes gives reach them."""
    T1 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    shear = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [1, 0, 1, 0]], np.float32)
    ok, _ = oracle.triangulate([0, 0, 1], [0, 0, 1], T1, shear)
    assert not ok
    cam6 = [458.654, 457.296, 367.215, 248.375, 0.11, 458.654 * 0.11]
    sf = 1.2 ** np.arange(8)
    a = dict(Tcw=T1, Twc=T1, Ow=[0, 0, 0], x=cam6[2], y=cam6[3], octave=0)
    b = dict(Tcw=shear, Twc=T1, Ow=[1, 0, 0], x=cam6[2], y=cam6[3], octave=0)
    assert oracle.decide(cam6, [a, b], sf, sf * sf)[0] == ST["TRIANGULATE_FALSE"]
    # a real pair and its point, but keyframe 2's centre given as the point itself
    T2 = np.array([[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    W2 = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    X = np.array([0.4, -0.2, 5.0])
    uv = lambda Xc: (cam6[0] * Xc[0] / Xc[2] + cam6[2], cam6[1] * Xc[1] / Xc[2] + cam6[3])
    a = dict(Tcw=T1, Twc=T1, Ow=[0, 0, 0], x=uv(X)[0], y=uv(X)[1], octave=0)
    b = dict(Tcw=T2, Twc=W2, Ow=[1, 0, 0], x=uv(X - [1, 0, 0])[0], y=uv(X - [1, 0, 0])[1], octave=0)
    st, x3D, _ = oracle.decide(cam6, [a, b], sf, sf * sf)
    assert st == ST["TRIANGULATED"] and np.abs(x3D - X).max() < 1e-3
    assert oracle.decide(cam6, [a, dict(b, Ow=x3D)], sf, sf * sf)[0] == ST["ZERO_DIST"]
    assert oracle.decide(cam6, [dict(a, Ow=x3D), b], sf, sf * sf)[0] == ST["ZERO_DIST"]


def test_accepted_points_are_the_scenes_points():
    """Where both keypoints are exact projections, a triangulated point lies within 1e-3 of the scene's; its normal, distances,
    descriptor and second observation follow from the scene."""
    for s, r in zip(corpus.scenes(), corpus.results()):
        t = r["tables"]
        exact = (r["status"] == ST["TRIANGULATED"]) & ~np.isin(s["category"], NOISY)
        assert exact.sum() >= 60, s["kind"]
        d = np.linalg.norm(t["Xw"][exact] - s["X"][exact], axis=1)
        print(s["kind"], "largest distance to the true point", d.max())
        assert d.max() <= 1e-3
        for p in range(s["npairs"]):
            Ow1 = s["poses"][p, 1].reshape(3, 4)[:, 3]
            for i1 in np.nonzero(np.isin(r["status"][p], NEW_MAP_POINT_CREATED))[0]:
                i2 = s["match12"][p, i1]
                assert t["img2"][p, i1] == s["img2"][p] and t["idx2"][p, i1] == i2
                src = s["desc"][s["img2"][p], i2] if s["kf2First"][p] else s["desc"][s["img1"][p], i1]
                assert np.array_equal(t["desc"][p, i1], src)
                dist = np.linalg.norm(t["Xw"][p, i1] - Ow1)
                assert abs(t["maxDist"][p, i1] - dist * s["scaleFactors"][s["octave"][s["img1"][p], i1]]) <= 1e-4 * dist
                assert abs(t["minDist"][p, i1] - t["maxDist"][p, i1] / s["scaleFactors"][-1]) <= 1e-5 * dist
                assert 0.5 < np.linalg.norm(t["normal"][p, i1]) <= 1 + 1e-6
                assert r["hasMP"][s["img1"][p], i1] == 1 and r["hasMP"][s["img2"][p], i2] == 1
        created = np.isin(r["status"], NEW_MAP_POINT_CREATED)
        assert r["hasMP"].sum() == created.sum() + sum(len(set(s["match12"][p][created[p]])) for p in range(s["npairs"]))
        assert (r["stats"][:, 0] == created.sum(1)).all()
        assert (r["stats"][:, 4] == np.isin(r["status"], [ST["STEREO1"], ST["STEREO2"]]).sum(1)).all()


def test_no_decision_of_the_corpus_sits_on_a_rounding_edge():
    """A second build of the oracle (-O3 -march=native -ffp-contract=fast: fused multiply-adds, another instruction order) decides every
    match of the corpus alike; this is what lets the GPU test allow no exception."""
    a, b = corpus.results(), corpus.results(oracle.OTHER_FLAGS)
    for s, x, y in zip(corpus.scenes(), a, b):
        assert np.array_equal(x["status"], y["status"]) and np.array_equal(x["stats"], y["stats"]), s["kind"]
        assert np.array_equal(x["hasMP"], y["hasMP"])
        assert np.abs(x["tables"]["Xw"] - y["tables"]["Xw"]).max() <= 1e-4


def test_match_entries_beyond_the_second_count_and_bad_rows_in_the_oracle():
    s = corpus.scenes()[0]
    A = oracle.arrays_of_scene(s)
    base = corpus.results()[0]
    m = s["match12"].copy()
    hit = np.nonzero(m[0] >= 0)[0][[1, 4]]
    m[0, hit] = [s["count"][s["img2"][0]], 2 ** 30]
    r = oracle.run(dict(A, match12=m))
    assert (r["status"][0, hit] == ST["NONE"]).all() and np.array_equal(r["status"][1:], base["status"][1:])
    keep = np.ones(s["cap"], bool); keep[hit] = False
    assert np.array_equal(r["status"][0, keep], base["status"][0, keep])
    r = oracle.run(A, row=np.array([0, 9, 2, 3], np.int32))
    assert (r["stats"][1] == -1).all() and np.array_equal(r["stats"][[0, 2, 3]], base["stats"][[0, 2, 3]])


def test_pair_gate():
    assert oracle.gate(False, [0, 0, 0], [0.1, 0, 0], 0.11, 0.0) and not oracle.gate(False, [0, 0, 0], [0.12, 0, 0], 0.11, 0.0)
    assert oracle.gate(True, [0, 0, 0], [0.1, 0, 0], 0.0, 10.5) and not oracle.gate(True, [0, 0, 0], [0.1, 0, 0], 0.0, 9.5)


def test_math_header_under_sanitizers(tmp_path):
    """tests/native/new_map_points_math_check.cc, a program of its own, with -fsanitize=address,undefined."""
    exe = str(tmp_path / "new_map_points_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "new_map_points_math_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    lines = out.stdout.splitlines()
    status = [ln.split()[1:] for ln in lines if ln.startswith("status ")]
    stats = [ln.split()[1:] for ln in lines if ln.startswith("stat ")]
    assert [n for n, _ in status] == list(NEW_MAP_POINT_STATUS) and [int(v) for _, v in status] == list(range(len(NEW_MAP_POINT_STATUS)))
    assert [n for n, _ in stats] == list(NEW_MAP_POINT_STATS) and [int(v) for _, v in stats] == list(range(len(NEW_MAP_POINT_STATS)))


def test_library_exports_the_entries():
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    assert os.path.exists(lib), "build() first"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT morb_create_new_map_points_batch\b", nm) and re.search(r"\bT morb_create_new_map_points_fisheye_batch\b", nm)


def test_python_front_is_there():
    from morb_slam_amd import ORBmatcher
    assert callable(ORBmatcher.CreateNewMapPoints) and callable(ORBmatcher.new_map_point_tables)
