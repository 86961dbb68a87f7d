"""KeyFrameDatabase place recognition on the GPU (morb_detect_n_best_candidates_batch, morb_detect_relocalization_candidates_batch)
against the CPU oracle (tests/native/keyframe_database_oracle.cc) on the scenes of tests/keyframe_database_corpus.py.  The reference's
arithmetic is a fixed sequence of IEEE adds, so everything is compared for EQUALITY: d_words, d_score as float bit patterns, the
candidate lists with their -1 padding and their counts."""
import numpy as np
import pytest
import torch

import keyframe_database_corpus as corpus
import keyframe_database_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.capi import ERR_INVALID, KP_DTYPE, MORB_OK, lib, ptr
from morb_slam_amd.synth import keyframe_database_connected_csr, make_vocabulary

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = corpus.N_CAND


@pytest.fixture(scope="module")
def m():
    o = ORBmatcher(0.8, True)
    yield o
    o.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pool(scene):
    return dict(bow=(_dev(scene["word"]), _dev(scene["value"]), _dev(scene["count"])), db_rank=_dev(scene["db_rank"]),
                covis=_dev(scene["covis"]), map_id=_dev(scene["map_id"]), flags=_dev(scene["flags"]))


def _n_best(m, scene, queries, prev=None, n=N):
    p = _pool(scene)
    cs, cn = keyframe_database_connected_csr(scene, queries)
    out = m.DetectNBestCandidates(_dev(np.asarray(queries, np.int32)), p["bow"], p["db_rank"], _dev(cs), _dev(cn), p["covis"], p["map_id"],
                                  p["flags"], n, prev_score=None if prev is None else _dev(np.asarray(prev, np.float32)))
    torch.cuda.synchronize()
    return dict(zip(("loop", "nLoop", "merge", "nMerge", "words", "score"), (t.cpu().numpy() for t in out)))


def _reloc(m, scene, queries, qmaps, prev=None):
    p = _pool(scene)
    out = m.DetectRelocalizationCandidates(_dev(np.asarray(queries, np.int32)), _dev(np.asarray(qmaps, np.int32)), p["bow"], p["db_rank"],
                                           p["covis"], p["map_id"], prev_score=None if prev is None else _dev(np.asarray(prev, np.float32)))
    torch.cuda.synchronize()
    return dict(zip(("cand", "nCand", "words", "score"), (t.cpu().numpy() for t in out)))


def _same(got, want, tag):
    for k, w in want.items():
        g = got[k]
        if k == "score":
            assert g.view(np.uint32).tobytes() == w.view(np.uint32).tobytes(), (tag, k, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5])
        else:
            assert np.array_equal(g, w), (tag, k, g, w)


NBEST_SCENES = ("base", "base_bad_map", "ties", "one_word", "empty_database", "no_shared_word", "all_connected", "all_bad", "at_threshold")


@pytest.mark.parametrize("name", NBEST_SCENES)
def test_n_best_equals_the_oracle(m, name):
    """Base: 70 keyframes (two waves of keyframes and a part, 18 workgroups of the intersection), cap 128, 20 to 100 words, two maps,
    covisibility rows of every length from 0 to 10, rows outside the database, bad keyframes, a bad map, five queries in one batch.
    Ties: groups of keyframes with identical vectors.  The degenerate scenes: nothing in the database, queries sharing no word,
    every keyframe connected, every keyframe bad, one-word vectors, a count exactly at minCommonWords (not scored)."""
    scene, queries = getattr(corpus, name)()
    want = oracle.expected_n_best(scene, queries, N)
    got = _n_best(m, scene, queries)
    _same(got, want, name)
    if name == "at_threshold":
        assert got["words"][0, 2] == 8 and got["score"][0, 2] == 0 and got["score"][0, 3] > 0   # eight common words of ten: stamped, not scored
    if name in ("empty_database", "no_shared_word", "all_connected"):
        assert (got["words"] == -1).all() and not got["nLoop"].any() and not got["nMerge"].any() and (got["loop"] == -1).all()


@pytest.mark.parametrize("name", NBEST_SCENES)
def test_relocalization_equals_the_oracle(m, name):
    """The same scenes through the second entry; every second query searches the other map, so entries whose best keyframe lies in
    another map than pMap are dropped (tests/test_keyframe_database_cpu.py checks that the corpus has them)."""
    scene, queries = getattr(corpus, name)()
    qmaps = corpus.reloc_maps(scene, queries)
    _same(_reloc(m, scene, queries, qmaps), oracle.expected_reloc(scene, queries, qmaps), name)


def test_stale_scores_carried_from_query_to_query(m):
    """d_score of one call is d_prevScore of the next, three queries, against ONE stateful oracle; then the hand-built scene in which
    a stamped, unscored neighbour decides the candidate with the score the query before left on it."""
    for build, reloc in ((corpus.stale, False), (corpus.stale, True), (corpus.stale_neighbour, False)):
        scene, queries = build()
        db, prev, stale_used = oracle.Database(scene), None, 0
        for q in queries:
            if reloc:
                g = _reloc(m, scene, [q], [scene["map_id"][q]], prev)
                c, qid = db.detect_reloc(q, scene["map_id"][q])
                assert g["nCand"][0] == len(c) and np.array_equal(g["cand"][0, :len(c)], c) and (g["cand"][0, len(c):] == -1).all()
            else:
                g = _n_best(m, scene, [q], prev)
                lo, me, qid = db.detect_n_best(q, N)
                assert g["nLoop"][0] == len(lo) and np.array_equal(g["loop"][0, :len(lo)], lo) and (g["loop"][0, len(lo):] == -1).all()
                assert g["nMerge"][0] == len(me) and np.array_equal(g["merge"][0, :len(me)], me) and (g["merge"][0, len(me):] == -1).all()
            words, score = db.device_view(int(reloc), qid)
            assert np.array_equal(g["words"][0], words) and g["score"][0].view(np.uint32).tobytes() == score.view(np.uint32).tobytes()
            if prev is not None:
                stale_used += int(((words > 0) & (score == prev) & (prev != 0)).sum())
            prev = g["score"][0]
        assert stale_used > 0, "no stamped keyframe kept an earlier score: the scene does not test the carry"
    scene, (q0, q1) = corpus.stale_neighbour()
    s0 = _n_best(m, scene, [q0])["score"][0]
    assert list(_n_best(m, scene, [q1], s0)["loop"][0]) == [3, -1, -1] and list(_n_best(m, scene, [q1])["loop"][0]) == [2, -1, -1]


def test_large_pool_beyond_the_lds_tier(m):
    """5000 keyframes > corpus.LDS_N = 4096: the sort lists of k_kfdb_select live in the handle's workspace, the bitonic sorts run on
    up to 8192 padded entries.  Both entries, two queries."""
    scene, queries = corpus.large()
    assert len(scene["count"]) > corpus.LDS_N
    _same(_n_best(m, scene, queries), oracle.expected_n_best(scene, queries, N), "large")
    qmaps = corpus.reloc_maps(scene, queries)
    _same(_reloc(m, scene, queries, qmaps), oracle.expected_reloc(scene, queries, qmaps), "large reloc")


def test_batch_of_n_equals_n_batches_of_one_and_null_outputs(m):
    scene, queries = corpus.ties()
    prev = np.random.default_rng(3).random(len(scene["count"])).astype(np.float32)
    whole = _n_best(m, scene, queries, prev)
    _same(whole, oracle.expected_n_best(scene, queries, N, prev), "ties on random entry scores")
    for k, q in enumerate(queries):
        one = _n_best(m, scene, [q], prev)
        for key in whole:
            assert np.array_equal(one[key][0], whole[key][k]), (key, k)
    # d_words / d_score NULL: the lists are the same
    p = _pool(scene)
    cs, cn = keyframe_database_connected_csr(scene, queries)
    nq, L = len(queries), lib()
    lo, me = torch.full((nq, N), -7, dtype=torch.int32, device=DEV), torch.full((nq, N), -7, dtype=torch.int32, device=DEV)
    nl, nm = torch.zeros(nq, dtype=torch.int32, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV)
    w, v, c = p["bow"]
    d_q, d_cs, d_cn, d_prev = _dev(queries), _dev(cs), _dev(cn), _dev(prev)
    rc = L.morb_detect_n_best_candidates_batch(m._h, nq, ptr(d_q), w.shape[0], w.shape[1], ptr(w), ptr(v), ptr(c), ptr(p["db_rank"]), ptr(d_cs),
                                               ptr(d_cn), ptr(p["covis"]), scene["ncovis"], ptr(p["map_id"]), ptr(p["flags"]), ptr(d_prev), N,
                                               ptr(lo), ptr(nl), ptr(me), ptr(nm), None, None, None)
    torch.cuda.synchronize()
    assert rc == MORB_OK and np.array_equal(lo.cpu().numpy(), whole["loop"]) and np.array_equal(me.cpu().numpy(), whole["merge"])
    assert np.array_equal(nl.cpu().numpy(), whole["nLoop"]) and np.array_equal(nm.cpu().numpy(), whole["nMerge"])


def test_argument_refusals_and_empty_calls(m):
    """MORB_ERR_INVALID for each condition, before any launch; nq == 0 and nimg == 0 are MORB_OK and write nothing."""
    scene, queries = corpus.at_threshold()
    p = _pool(scene)
    w, v, c = p["bow"]
    nimg, cap = w.shape
    cs, cn = keyframe_database_connected_csr(scene, queries)
    d_q, d_cs, d_cn, d_qm = _dev(queries), _dev(cs), _dev(cn), _dev(np.zeros(1, np.int32))
    out = [torch.full((8,), -7, dtype=torch.int32, device=DEV) for _ in range(4)]
    L = lib()

    def nbest(nq=1, nimg=nimg, cap=cap, ncovis=scene["ncovis"], n=N):
        return L.morb_detect_n_best_candidates_batch(m._h, nq, ptr(d_q), nimg, cap, ptr(w), ptr(v), ptr(c), ptr(p["db_rank"]), ptr(d_cs), ptr(d_cn),
                                                     ptr(p["covis"]), ncovis, ptr(p["map_id"]), ptr(p["flags"]), None, n, ptr(out[0]), ptr(out[1]),
                                                     ptr(out[2]), ptr(out[3]), None, None, None)

    def reloc(nq=1, nimg=nimg, cap=cap, ncovis=scene["ncovis"]):
        return L.morb_detect_relocalization_candidates_batch(m._h, nq, ptr(d_q), ptr(d_qm), nimg, cap, ptr(w), ptr(v), ptr(c), ptr(p["db_rank"]),
                                                             ptr(p["covis"]), ncovis, ptr(p["map_id"]), None, ptr(out[0]), ptr(out[1]), None, None, None)

    for f in (nbest, reloc):
        for bad in (dict(nq=-1), dict(nimg=-1), dict(cap=0), dict(cap=-3), dict(ncovis=-1)):
            assert f(**bad) == ERR_INVALID, (f.__name__, bad)
        assert f(nq=0) == MORB_OK and f(nimg=0) == MORB_OK
    assert nbest(n=0) == ERR_INVALID and nbest(n=-2) == ERR_INVALID
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out)          # nothing was written by any of these calls
    assert nbest() == MORB_OK and reloc() == MORB_OK
    torch.cuda.synchronize()


def test_chain_from_descriptors_to_search_by_bow_on_the_device(m):
    """bow_transform -> bow_vector -> DetectNBestCandidates -> SearchByBoWKeyFrames on one stream: the candidate tensor goes on as
    kf2_img without leaving the device.  The pool: 12 images of 300 descriptors, four groups of three near copies (a few bits
    flipped), so that the copies of the query's group are its loop candidates.  The BoW vectors are read back only to drive the
    oracle, whose candidates, uploaded, must give the same matches."""
    rng = np.random.default_rng(8)
    k, Lv, nimg, cap, n = 10, 3, 12, 320, 300
    vd, vf = make_vocabulary(k, Lv, seed=4)
    base = rng.integers(0, 256, (4, n, 32), dtype=np.uint8)
    desc = np.zeros((nimg, cap, 32), np.uint8)
    for i in range(nimg):
        flips = np.packbits(rng.random((n, 256)) < 0.01, axis=1)
        desc[i, :n] = base[i // 3] ^ flips
    kps = np.zeros((nimg, cap), KP_DTYPE)
    kps["x"], kps["y"], kps["angle"] = rng.uniform(20, 700, cap), rng.uniform(20, 460, cap), rng.uniform(0, 360, cap)   # every image alike: no rotation
    d_desc, d_cnt = _dev(desc), _dev(np.full(nimg, n, np.int32))
    d_kps = _dev(kps.view(np.uint8).reshape(nimg, cap, KP_DTYPE.itemsize))
    weight = rng.uniform(0.5, 9.0, len(vd))
    has = _dev(np.ones((nimg, cap), np.uint8))
    st = torch.cuda.Stream()
    scene = dict(db_rank=np.arange(nimg, dtype=np.int32), covis=np.full((nimg, 2), -1, np.int32), map_id=np.zeros(nimg, np.int32),
                 flags=np.zeros(nimg, np.uint8), connected=[np.zeros(0, np.int32)] * nimg, nwords_voc=len(vd), nmaps=1, cap=cap, ncovis=2)
    scene["db_rank"][0] = -1                                           # the query is not in the database yet
    queries = np.array([0], np.int32)
    cs, cn = keyframe_database_connected_csr(scene, queries)
    d_vd, d_vf, d_w, d_q, d_cs, d_cn = _dev(vd), _dev(vf), _dev(weight), _dev(queries), _dev(cs), _dev(cn)
    d_rank, d_cov, d_map, d_flags = _dev(scene["db_rank"]), _dev(scene["covis"]), _dev(scene["map_id"]), _dev(scene["flags"])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        leaf, node = m.bow_transform(d_desc, d_cnt, d_vd, d_vf, k, Lv, 1, stream=st.cuda_stream)
        bow = m.bow_vector(leaf, d_cnt, d_w, stream=st.cuda_stream)
        det = m.DetectNBestCandidates(d_q, bow, d_rank, d_cs, d_cn, d_cov, d_map, d_flags, 2, stream=st.cuda_stream)
        kf2 = det[0].reshape(-1)                                       # the two loop candidates, still on the device
        kf1 = d_q.expand(2).contiguous()
        m12, nm = m.SearchByBoWKeyFrames(kf1, kf2, d_kps, d_desc, node, d_cnt, has, stream=st.cuda_stream)
    st.synchronize()
    scene["word"], scene["value"], scene["count"] = (t.cpu().numpy() for t in bow)
    want = oracle.expected_n_best(scene, queries, 2)
    assert want["nLoop"][0] == 2 and set(want["loop"][0].tolist()) == {1, 2}, want["loop"]
    assert np.array_equal(det[0].cpu().numpy(), want["loop"]) and np.array_equal(det[4].cpu().numpy(), want["words"])
    m12o, nmo = m.SearchByBoWKeyFrames(_dev(np.array([0, 0], np.int32)), _dev(want["loop"][0]), d_kps, d_desc, node, d_cnt, has)
    torch.cuda.synchronize()
    assert np.array_equal(m12.cpu().numpy(), m12o.cpu().numpy()) and np.array_equal(nm.cpu().numpy(), nmo.cpu().numpy())
    assert (nm.cpu().numpy() > 50).all()
