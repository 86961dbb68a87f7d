"""LocalMapping::CreateNewMapPoints on the GPU (morb_create_new_map_points_batch and its KannalaBrandt8 form) against the CPU oracle
(tests/native/new_map_points_oracle.cc) on the corpus of tests/new_map_points_corpus.py.  Exactly, for every match and with no case
left out: status, stats, the updated hasMP, descriptors, img2 and idx2, and every table entry that is not an accepted point (the
tables start from a sentinel).  Within the project's 1e-4 gate: Xw (relative to max(1, |X|)), the normal, and the two distances
(relative to max(1, distance)).  tests/test_new_map_points_cpu.py shows that a second build of the oracle decides the corpus alike,
which is why no exception is allowed here.  Also: a batch against each pair alone and a rerun, byte for byte; a caller's stream; one
pair at cap 4500 with a dense table; entries beyond keyframe 2's count; the argument refusals; and the chain SearchForTriangulation ->
CreateNewMapPoints -> SearchForTriangulation -> Fuse on one stream."""
import contextlib

import numpy as np
import pytest
import torch

import new_map_points_corpus as corpus
import new_map_points_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.capi import ERR_INVALID, ERR_UNSUPPORTED, KP_DTYPE, lib, ptr
from morb_slam_amd.matcher import NEW_MAP_POINT_CREATED, NEW_MAP_POINT_STATUS
from morb_slam_amd.synth import _quat_from_R, make_new_map_points_scene, new_map_points_frame_params, pack_new_map_points_scene

pytestmark = pytest.mark.gpu

GATE = 1e-4
SENTINEL = 0xA5
DEV = "cuda:0"
ST = {n: k for k, n in enumerate(NEW_MAP_POINT_STATUS)}
FLOATS, EXACT = ("Xw", "normal", "maxDist", "minDist"), ("desc", "img2", "idx2")


@pytest.fixture(scope="module")
def matcher():
    m = ORBmatcher(0.6, False, device=0)
    yield m
    m.close()


@contextlib.contextmanager
def _callers_stream():
    """A stream that is the caller's and not the matcher's: a second handle's own, wrapped for torch and destroyed with that handle, so
    that the tests leave no stream behind in the process (a pooled torch.cuda.Stream() is never released and keeps a hardware queue)."""
    other = ORBmatcher(0.6, False, device=0)
    try:
        yield torch.cuda.ExternalStream(int(lib().morb_matcher_stream(other._h)))
    finally:
        torch.cuda.synchronize()
        other.close()


def _subset(scene, pairs):
    """The scene restricted to some of its pairs (the image pool stays whole)."""
    s = dict(scene, npairs=len(pairs))
    for k in ("img1", "img2", "match12", "poses", "kf2First", "R12", "t12", "ep"):
        s[k] = np.ascontiguousarray(scene[k][pairs])
    return s


def _run(matcher, scene, stream=None, match12=None, row=None, nrows=None, hasMP=None):
    """One call; the tables start from the sentinel.  Returns numpy: status, stats, tables, hasMP."""
    t = pack_new_map_points_scene(scene, DEV)
    nrows = scene["npairs"] if nrows is None else nrows
    tables = matcher.new_map_point_tables(nrows, scene["cap"], DEV)
    for v in tables.values():
        v.view(torch.uint8).fill_(SENTINEL)
    if match12 is not None:
        t["match12"] = torch.from_numpy(match12).to(DEV)
    if row is not None:
        t["row"] = torch.from_numpy(np.asarray(row, np.int32)).to(DEV)
    if hasMP is not None:
        t["hasMP"] = torch.from_numpy(hasMP.copy()).to(DEV)
    torch.cuda.synchronize()
    status, stats = matcher.CreateNewMapPoints(
        new_map_points_frame_params(scene), t["img1"], t["img2"], t["kps"], t["desc"], t["count"], t["match12"], scene["poses"],
        scene["kf2First"], t["row"], tables, t["hasMP"], uRight=t["uRight"], depth=t["depth"], kpsRaw=t["kpsRaw"],
        ratioFactor=scene["ratioFactor"], mbInertial=scene["inertial"], mbFarPoints=scene["farPoints"], mThFarPoints=scene["thFarPoints"],
        nLeft1=t["nLeft1"], nLeft2=t["nLeft2"], camL8=scene["camL8"] if scene["rig"] else None,
        camR8=scene["camR8"] if scene["rig"] else None, stream=stream)
    torch.cuda.synchronize()
    return dict(status=status.cpu().numpy(), stats=stats.cpu().numpy(), tables={k: v.cpu().numpy() for k, v in tables.items()},
                hasMP=t["hasMP"].cpu().numpy())


def _oracle(scene, match12=None, row=None, nrows=None, hasMP=None):
    A = oracle.arrays_of_scene(scene)
    if match12 is not None:
        A["match12"] = match12
    nrows = scene["npairs"] if nrows is None else nrows
    return oracle.run(A, tables=oracle.empty_tables(nrows, scene["cap"], fill=SENTINEL), row=row, nrows=nrows,
                      hasMP=None if hasMP is None else hasMP.copy())


def _compare(tag, g, o, dev=None):
    """Everything equal but the four float tables, which are within GATE at accepted points and untouched (the sentinel's bytes) elsewhere."""
    assert np.array_equal(g["status"], o["status"]), (tag, np.argwhere(g["status"] != o["status"])[:5])
    assert np.array_equal(g["stats"], o["stats"]), (tag, g["stats"], o["stats"])
    assert np.array_equal(g["hasMP"], o["hasMP"]), tag
    for k in EXACT:
        assert g["tables"][k].tobytes() == o["tables"][k].tobytes(), (tag, k)
    # which row an accepted point went to: the oracle's img2 table is no longer the sentinel there
    acc = o["tables"]["img2"].view(np.uint8).reshape(o["tables"]["img2"].shape + (4,))[..., 0] != SENTINEL
    worst, nbits, nvals = 0.0, 0, 0
    for k in FLOATS:
        a, b = g["tables"][k], o["tables"][k]
        assert a[~acc].tobytes() == b[~acc].tobytes(), (tag, k, "a row that was not accepted was written")
        if not acc.any():
            continue
        x, y = a[acc].astype(np.float64), b[acc].astype(np.float64)
        if k == "Xw":
            d = np.linalg.norm(x - y, axis=1) / np.maximum(1.0, np.linalg.norm(y, axis=1))
        elif k == "normal":
            d = np.abs(x - y).max(axis=1)
        else:
            d = np.abs(x - y) / np.maximum(1.0, np.abs(y))
        worst = max(worst, float(d.max()))
        nbits += int((a[acc].view(np.uint32) != b[acc].view(np.uint32)).sum())
        nvals += a[acc].size
        assert d.max() <= GATE, (tag, k, float(d.max()))
    if dev is not None:
        dev.append((worst, nbits, nvals))
    return worst, nbits, nvals


def test_corpus_matches_oracle(matcher):
    dev = []
    for scene, o in zip(corpus.scenes(), corpus.results()):
        g = _run(matcher, scene)
        # the shared results start from zeros, these from the sentinel: the decisions are the shared ones, the tables are compared with a
        # sentinel twin
        o2 = _oracle(scene)
        assert np.array_equal(o2["status"], o["status"]) and np.array_equal(o2["stats"], o["stats"])
        w, nb, nv = _compare(scene["kind"], g, o2, dev)
        print(f"{scene['kind']}: created {int(o['stats'][:, 0].sum())}, largest deviation {w:.3e}, {nb} of {nv} float values differ in bits")
    print(f"largest deviation on the device: {max(d[0] for d in dev):.3e}; values that differ in bits: {sum(d[1] for d in dev)} of "
          f"{sum(d[2] for d in dev)}")
    h = corpus.status_histogram()
    assert all(h[ST[n]] > 0 for n in NEW_MAP_POINT_STATUS if n not in ("NONE", "TRIANGULATE_FALSE", "ZERO_DIST"))


def test_batch_equals_each_pair_alone_and_rerun(matcher):
    for scene in corpus.scenes():
        a, b = _run(matcher, scene), _run(matcher, scene)
        for k in ("status", "stats", "hasMP"):
            assert a[k].tobytes() == b[k].tobytes(), (scene["kind"], k)
        for k in a["tables"]:
            assert a["tables"][k].tobytes() == b["tables"][k].tobytes(), (scene["kind"], k)
        has = np.zeros_like(a["hasMP"])
        for p in range(scene["npairs"]):
            one = _run(matcher, _subset(scene, [p]))
            assert one["status"][0].tobytes() == a["status"][p].tobytes() and one["stats"][0].tobytes() == a["stats"][p].tobytes()
            for k in a["tables"]:
                assert one["tables"][k][0].tobytes() == a["tables"][k][p].tobytes(), (scene["kind"], p, k)
            has |= one["hasMP"]
        assert np.array_equal(has, a["hasMP"])


def test_callers_stream_rows_and_bad_indices(matcher):
    """On a caller's stream; pairs writing rows of a larger table in another order; a pair whose row lies outside the table."""
    scene = corpus.scenes()[1]
    with _callers_stream() as s, torch.cuda.stream(s):
        g = _run(matcher, scene, stream=s.cuda_stream, row=[5, 0, 3, 1], nrows=6)
    _compare("stream", g, _oracle(scene, row=np.array([5, 0, 3, 1], np.int32), nrows=6))
    g = _run(matcher, scene, row=[0, 7, -1, 3], nrows=4)
    o = _oracle(scene, row=np.array([0, 7, -1, 3], np.int32), nrows=4)
    assert (o["stats"][[1, 2]] == -1).all() and (o["stats"][[0, 3], 0] > 0).all()
    _compare("bad rows", g, o)


def test_largest_compaction_cap_4500(matcher):
    """One pair, 4500 features each, every feature of keyframe 1 matched: 18 passes of the compaction, 4500 matches over 256 threads."""
    scene = make_new_map_points_scene(seed=11, kind="mono", npairs=1, cap=4500, dense=True)
    assert (scene["match12"] >= 0).sum() == 4500 and scene["count"].tolist() == [4500, 4500]
    o = _oracle(scene)
    assert o["stats"][0, 0] > 1000
    w, nb, nv = _compare("cap 4500", _run(matcher, scene), o)
    print(f"cap 4500: created {int(o['stats'][0, 0])}, largest deviation {w:.3e}, {nb} of {nv} float values differ in bits")


def test_an_entry_beyond_the_second_count_is_no_match(matcher):
    scene = corpus.scenes()[0]
    m = scene["match12"].copy()
    for p in range(scene["npairs"]):
        hit = np.nonzero(m[p] >= 0)[0][[0, 3, 9]]
        m[p, hit] = [scene["count"][scene["img2"][p]], scene["cap"] + 7, 2 ** 30]
    # ... and rows beyond keyframe 1's count are not read as matches
    m[0, scene["count"][scene["img1"][0]]:] = 0
    o = _oracle(scene, match12=m)
    base = corpus.results()[0]
    assert o["stats"][:, 0].sum() < base["stats"][:, 0].sum()
    _compare("beyond", _run(matcher, scene, match12=m), o)


def test_hasmp_is_updated_in_place_on_top_of_what_is_there(matcher):
    scene = corpus.scenes()[2]
    rng = np.random.default_rng(4)
    has = (rng.random((scene["nimg"], scene["cap"])) < 0.2).astype(np.uint8) * 3
    g, o = _run(matcher, scene, hasMP=has), _oracle(scene, hasMP=has)
    _compare("hasMP", g, o)
    assert (g["hasMP"][has > 0] == np.where(o["hasMP"][has > 0] == 1, 1, 3)).all() and (g["hasMP"] == 1).sum() > 50


def test_invalid_arguments_are_refused_before_any_launch(matcher):
    scene = corpus.scenes()[1]
    t = pack_new_map_points_scene(scene, DEV)
    P = new_map_points_frame_params(scene)
    tables = matcher.new_map_point_tables(scene["npairs"], scene["cap"], DEV)
    status = torch.zeros((scene["npairs"], scene["cap"]), dtype=torch.int32, device=DEV)
    stats = torch.zeros((scene["npairs"], 5), dtype=torch.int32, device=DEV)
    poses, first = np.ascontiguousarray(scene["poses"], np.float32), np.ascontiguousarray(scene["kf2First"], np.uint8)
    L = lib()
    import ctypes as C

    def call(npairs=scene["npairs"], cap=scene["cap"], nrows=scene["npairs"], depth=t["depth"], far=(1, 30.0), poses_=poses, P_=P, hasMP=t["hasMP"]):
        return L.morb_create_new_map_points_batch(
            matcher._h, C.byref(P_), npairs, ptr(t["img1"]), ptr(t["img2"]), scene["nimg"], cap, ptr(t["count"]), ptr(t["kps"]), ptr(t["kpsRaw"]),
            ptr(t["desc"]), ptr(t["uRight"]), ptr(depth), ptr(t["match12"]), ptr(poses_), ptr(first), scene["ratioFactor"], 1, far[0], far[1],
            ptr(status), ptr(stats), nrows, ptr(t["row"]), ptr(tables["Xw"]), ptr(tables["normal"]), ptr(tables["maxDist"]),
            ptr(tables["minDist"]), ptr(tables["desc"]), ptr(tables["img2"]), ptr(tables["idx2"]), ptr(hasMP), None)
    assert call(npairs=0) == ERR_INVALID
    assert call(cap=0) == ERR_INVALID
    assert call(nrows=0) == ERR_INVALID
    assert call(depth=None) == ERR_INVALID          # mvuRight without mvDepth
    assert call(far=(1, 0.0)) == ERR_INVALID        # mbFarPoints without a threshold
    assert call(poses_=None) == ERR_INVALID
    assert call(hasMP=None) == ERR_INVALID
    assert call(cap=40000) == ERR_UNSUPPORTED
    bad = new_map_points_frame_params(scene)
    bad.nlevels = 17
    assert call(P_=bad) == ERR_INVALID
    rc = L.morb_create_new_map_points_fisheye_batch(
        matcher._h, C.byref(P), scene["npairs"], ptr(t["img1"]), ptr(t["img2"]), None, None, scene["nimg"], scene["cap"], ptr(t["count"]),
        ptr(t["kps"]), ptr(t["desc"]), None, None, ptr(t["match12"]), ptr(poses), ptr(first), scene["ratioFactor"], 1, 0, 0.0, ptr(status),
        ptr(stats), scene["npairs"], ptr(t["row"]), ptr(tables["Xw"]), ptr(tables["normal"]), ptr(tables["maxDist"]), ptr(tables["minDist"]),
        ptr(tables["desc"]), ptr(tables["img2"]), ptr(tables["idx2"]), ptr(t["hasMP"]), None)
    assert rc == ERR_INVALID
    torch.cuda.synchronize()
    assert not status.any() and not stats.any() and not t["hasMP"].any() and not tables["Xw"].any()   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), corpus.results()[1]["stats"])


def test_chain_search_create_search_fuse_on_one_stream(matcher):
    """morb_search_for_triangulation_batch -> morb_create_new_map_points_batch -> a second search on the same d_hasMP ->
    morb_fuse_batch on the produced table (every accepted point into the neighbour it was seen in), on one stream with no host copy in
    between.  Afterwards the intermediates are downloaded and each stage's oracle is run on the previous stage's device output."""
    import oracle_lib as O
    scene = corpus.scenes()[0]
    t = pack_new_map_points_scene(scene, DEV)
    P = new_map_points_frame_params(scene)
    npairs, cap, nimg = scene["npairs"], scene["cap"], scene["nimg"]
    node = torch.from_numpy(scene["node"]).to(DEV)
    tables = matcher.new_map_point_tables(npairs, cap, DEV)
    T7, Ow = np.zeros((npairs, 7), np.float32), np.zeros((npairs, 3), np.float32)
    for p in range(npairs):
        T2 = scene["poses"][p, 2].reshape(3, 4).astype(np.float64)
        T7[p], Ow[p] = np.concatenate([_quat_from_R(T2[:, :3]), T2[:, 3]]), scene["poses"][p, 3].reshape(3, 4)[:, 3]
    dT7, dOw = torch.from_numpy(T7).to(DEV), torch.from_numpy(Ow).to(DEV)
    nMP = torch.full((npairs,), cap, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with _callers_stream() as s, torch.cuda.stream(s):
        st = s.cuda_stream
        m12, nm = matcher.SearchForTriangulation(P, t["img1"], t["img2"], t["kps"], t["desc"], node, t["count"], t["hasMP"], None,
                                                 scene["R12"], scene["t12"], scene["ep"], stream=st)
        status, stats = matcher.CreateNewMapPoints(P, t["img1"], t["img2"], t["kps"], t["desc"], t["count"], m12, scene["poses"],
                                                   scene["kf2First"], t["row"], tables, t["hasMP"], ratioFactor=scene["ratioFactor"],
                                                   mbFarPoints=True, mThFarPoints=scene["thFarPoints"], stream=st)
        m12b, nmb = matcher.SearchForTriangulation(P, t["img1"], t["img2"], t["kps"], t["desc"], node, t["count"], t["hasMP"], None,
                                                   scene["R12"], scene["t12"], scene["ep"], stream=st)
        valid = (tables["img2"] >= 0).to(torch.uint8)
        bi, bd = matcher.Fuse(P, t["img2"], t["kps"], t["desc"], t["count"], None, dT7, dOw, nMP, valid, tables["Xw"], tables["normal"],
                              tables["maxDist"], tables["minDist"], tables["desc"], th=3.0, stream=st)
        s.synchronize()
    m12, m12b, bi, bd = (x.cpu().numpy() for x in (m12, m12b, bi, bd))
    kps = oracle.arrays_of_scene(scene)["kps"]
    sig, sf, K = [float(v) for v in scene["levelSigma2"]], [float(v) for v in scene["scaleFactors"]], [P.fx, P.fy, P.cx, P.cy]
    zero = np.zeros((nimg, cap), np.uint8)

    def search(has, p):
        a, b = scene["img1"][p], scene["img2"][p]
        na, nb = scene["count"][a], scene["count"][b]
        return O.search_for_triangulation(kps[a, :na], scene["desc"][a, :na], scene["node"][a, :na], has[a, :na], None, kps[b, :nb],
                                          scene["desc"][b, :nb], scene["node"][b, :nb], has[b, :nb], None, sig, sf, K, scene["R12"][p],
                                          scene["t12"][p], scene["ep"][p], False, False, False)
    for p in range(npairs):
        r, me = search(zero, p)
        assert int(nm[p]) == r and np.array_equal(m12[p, :len(me)], me), p
    assert int(nm.sum()) >= 60
    o = oracle.run(dict(oracle.arrays_of_scene(scene), match12=m12, inertial=False))
    g = dict(status=status.cpu().numpy(), stats=stats.cpu().numpy(), tables={k: v.cpu().numpy() for k, v in tables.items()},
             hasMP=t["hasMP"].cpu().numpy())
    created = np.isin(o["status"], NEW_MAP_POINT_CREATED)
    assert np.array_equal(g["status"], o["status"]) and np.array_equal(g["stats"], o["stats"]) and np.array_equal(g["hasMP"], o["hasMP"])
    for k in EXACT:
        assert np.array_equal(g["tables"][k], o["tables"][k]), k
    for k in FLOATS:
        assert np.abs(g["tables"][k][created] - o["tables"][k][created]).max() <= GATE * max(1.0, np.abs(o["tables"][k][created]).max()), k
    assert created.sum() >= 40
    # the second search: the oracle's search on the downloaded hasMP; no feature that received a point is matched again
    for p in range(npairs):
        r, me = search(g["hasMP"], p)
        assert int(nmb[p]) == r and np.array_equal(m12b[p, :len(me)], me), p
        i1 = np.nonzero(m12b[p] >= 0)[0]
        assert not g["hasMP"][scene["img1"][p], i1].any() and not g["hasMP"][scene["img2"][p], m12b[p, i1]].any()
        assert not (created[p] & (m12b[p] >= 0)).any()
    # Fuse on the produced table, against its oracle on the downloaded table
    invS = (1.0 / scene["levelSigma2"]).astype(np.float32)
    hits = 0
    for p in range(npairs):
        b = scene["img2"][p]; nb = scene["count"][b]
        Fo = O.make_frame(P, kps[b, :nb], scene["desc"][b, :nb], None)
        tb = g["tables"]
        ei, ed = O.fuse_search(Fo, invS, T7[p], Ow[p], (tb["img2"][p] >= 0), tb["Xw"][p], tb["normal"][p], tb["maxDist"][p], tb["minDist"][p],
                               tb["desc"][p], 3.0, False)
        assert np.array_equal(bi[p], ei) and np.array_equal(bd[p], ed), p
        # A new point projects onto the keypoint it was triangulated from, whose descriptor is within a few bits of the point's; any
        # other feature's is random (a Hamming distance near 128, TH_LOW is 50).  So where Fuse finds a feature, it is that one.  It
        # finds none where the keypoint's octave is not the level Fuse predicts from the distance, which the scene does not arrange.
        found = created[p] & (ei >= 0)
        assert np.array_equal(ei[found], tb["idx2"][p][found]), p
        hits += int(found.sum())
    assert hits > 0
