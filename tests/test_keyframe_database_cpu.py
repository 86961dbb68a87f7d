"""KeyFrameDatabase place recognition without a GPU: the CPU oracle (tests/native/keyframe_database_oracle.cc, an inverted file walked
as the reference walks it) against an independent numpy brute force that keeps NO inverted file and orders the sharing keyframes by
(rank in the query of the first common word, add rank), which is the equivalence the kernels rest on; the score against the dense L1
distance; the stale-score and connected-keyframe rules; include/morb/keyframe_database_math.h under sanitizers in a stand-alone
program; the C++ adapter against mock reference types; the header's declarations and the library's exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import keyframe_database_corpus as corpus
import keyframe_database_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SYMBOLS = ("morb_detect_n_best_candidates_batch", "morb_detect_relocalization_candidates_batch")


def min_common_words(m):
    return int(np.float32(m) * np.float32(0.8))


def brute_force(scene, q, prev, reloc=False, qmap=None, N=corpus.N_CAND):
    """One query on the entry scores `prev`, with no inverted file.  -> dict(sharing, words, score, and loop / merge or cand)."""
    n = len(scene["count"])
    rows = [dict(zip(scene["word"][k, :scene["count"][k]].tolist(), scene["value"][k, :scene["count"][k]].tolist())) for k in range(n)]
    qwords = sorted(rows[q])
    qrank = {w: r for r, w in enumerate(qwords)}
    connected = set() if reloc else set(scene["connected"][q].tolist())
    words, first = np.full(n, -1, np.int32), {}
    for k in range(n):
        if scene["db_rank"][k] < 0 or k in connected:
            continue
        common = [w for w in sorted(rows[k]) if w in qrank]
        if common:
            words[k], first[k] = len(common), qrank[common[0]]
    sharing = sorted(first, key=lambda k: (first[k], scene["db_rank"][k]))
    score = np.array(prev, np.float32).copy()
    out = dict(sharing=np.array(sharing, np.int32), words=words, score=score)
    empty = np.zeros(0, np.int32)
    out.update(dict(cand=empty) if reloc else dict(loop=empty, merge=empty))
    if not sharing:
        return out
    minc = min_common_words(words.max())
    scored = [k for k in sharing if words[k] > minc]
    for k in scored:
        s = 0.0
        for w in sorted(rows[k]):
            if w in qrank:
                s += abs(rows[q][w] - rows[k][w]) - abs(rows[q][w]) - abs(rows[k][w])   # Python floats: the same IEEE doubles
        score[k] = np.float32(-s / 2.0)
    acc = []
    best_acc = np.float32(0)
    for k in scored:
        best, a, pb = score[k], score[k], k
        for nb in scene["covis"][k]:
            if nb < 0 or words[nb] < 0:
                continue
            a = np.float32(a + score[nb])
            if score[nb] > best:
                pb, best = int(nb), score[nb]
        acc.append((a, pb))
        if a > best_acc:
            best_acc = a
    seen = set()
    if reloc:
        cand = []
        for a, pb in acc:
            if a > np.float32(np.float32(0.75) * best_acc):
                if scene["map_id"][pb] != qmap:
                    continue
                if pb not in seen:
                    cand.append(pb)
                    seen.add(pb)
        out["cand"] = np.array(cand, np.int32)
        return out
    order = sorted(range(len(acc)), key=lambda i: -float(acc[i][0]))   # sorted() is stable, as list::sort is
    loop, merge, qm = [], [], scene["map_id"][q]
    for i in order:
        pb = acc[i][1]
        if scene["flags"][pb] & 1:
            continue
        if pb not in seen:
            if scene["map_id"][pb] == qm and len(loop) < N:
                loop.append(pb)
            elif scene["map_id"][pb] != qm and len(merge) < N and not scene["flags"][pb] & 2:
                merge.append(pb)
            seen.add(pb)
    out["loop"], out["merge"] = np.array(loop, np.int32), np.array(merge, np.int32)
    return out


SCENES = ("base", "base_bad_map", "ties", "one_word", "empty_database", "no_shared_word", "all_connected", "all_bad", "at_threshold")


@pytest.mark.parametrize("name", SCENES)
def test_oracle_equals_the_brute_force_without_an_inverted_file(name):
    """Both detections, every query of the scene, statefully: the oracle keeps its scores from query to query and the brute force is
    given them.  The sharing list, the counts, the float scores (bit patterns) and the candidate lists are equal."""
    scene, queries = getattr(corpus, name)()
    n = len(scene["count"])
    for reloc in (False, True):
        db = oracle.Database(scene)
        qmaps = corpus.reloc_maps(scene, queries)
        nshare = ncand = 0
        for k, q in enumerate(queries):
            prev = db.state(int(reloc))[2]
            want = brute_force(scene, int(q), prev, reloc=reloc, qmap=int(qmaps[k]))
            if reloc:
                cand, qid = db.detect_reloc(q, qmaps[k])
                assert np.array_equal(cand, want["cand"]), (name, q)
                ncand += len(cand)
            else:
                lo, me, qid = db.detect_n_best(q, corpus.N_CAND)
                assert np.array_equal(lo, want["loop"]) and np.array_equal(me, want["merge"]), (name, q, lo, want["loop"], me, want["merge"])
                ncand += len(lo) + len(me)
            assert np.array_equal(db.last_sharing(), want["sharing"]), (name, q)
            words, score = db.device_view(int(reloc), qid)
            assert np.array_equal(words, want["words"]), (name, q)
            assert score.tobytes() == want["score"].tobytes(), (name, q)
            nshare += len(want["sharing"])
        print(f"{name} reloc={reloc}: {nshare} sharing, {ncand} candidates over {len(queries)} queries of {n} keyframes")
        if name in ("base", "ties"):
            assert nshare >= 30 * len(queries) and ncand >= (2 if reloc else len(queries))
        if name in ("empty_database", "no_shared_word", "all_connected") and not (reloc and name == "all_connected"):
            assert ncand == 0 and nshare == 0
        if name == "all_bad" and not reloc:
            assert ncand == 0 and nshare > 0


def test_the_corpus_reaches_every_rule():
    """What the scenes must hold, on the oracle's results, so that no test passes on a one-sided corpus."""
    scene, queries = corpus.base()
    e = oracle.expected_n_best(scene, queries, corpus.N_CAND)
    assert (e["nLoop"] > 0).any() and (e["nMerge"] > 0).any()
    so, qo = corpus.one_word()
    eo, allo = oracle.expected_n_best(so, qo, corpus.N_CAND), oracle.expected_n_best(so, qo, len(so["count"]))
    assert ((eo["nLoop"] == corpus.N_CAND) & (allo["nLoop"] > corpus.N_CAND)).any()      # full lists that more candidates would have entered
    assert ((eo["nMerge"] == corpus.N_CAND) & (allo["nMerge"] > corpus.N_CAND)).any()
    assert (scene["db_rank"] < 0).sum() >= 5 and (scene["flags"] & 1).sum() >= 2 and (scene["covis"][:, 0] < 0).any() and (scene["covis"][:, -1] >= 0).any()
    scored = (e["words"] > 0) & (e["score"] > 0)
    assert ((e["words"] > 0) & ~scored).any() and scored.sum() >= 2 * len(queries)
    sb, qb = corpus.base_bad_map()
    eb = oracle.expected_n_best(sb, qb, corpus.N_CAND)
    assert any(eb["nMerge"][k] == 0 and e["nMerge"][k] > 0 for k in range(len(qb)) if sb["map_id"][qb[k]] == 0)
    r = oracle.expected_reloc(scene, queries, scene["map_id"][queries])
    r2 = oracle.expected_reloc(scene, queries, corpus.reloc_maps(scene, queries))
    assert (r["nCand"] > 0).sum() >= 3 and (r2["nCand"] < r["nCand"]).any()     # entries whose best keyframe lies in another map are dropped
    st, qt = corpus.ties()
    et = oracle.expected_n_best(st, qt, corpus.N_CAND)
    tied = 0
    for k in range(len(qt)):
        sc = et["score"][k][et["words"][k] > 0]
        sc = sc[sc > 0]
        tied += len(sc) - len(np.unique(sc))
    assert tied >= 3
    sl, ql = corpus.large()
    assert len(sl["count"]) > corpus.LDS_N


def test_score_is_the_l1_distance_and_one_on_itself():
    scene, _ = corpus.base()
    rng = np.random.default_rng(5)
    V = np.zeros((len(scene["count"]), scene["nwords_voc"]))
    for k, c in enumerate(scene["count"]):
        V[k, scene["word"][k, :c]] = scene["value"][k, :c]
    for a, b in rng.integers(0, len(V), (200, 2)):
        s = oracle.score(scene["word"][a, :scene["count"][a]], scene["value"][a, :scene["count"][a]],
                         scene["word"][b, :scene["count"][b]], scene["value"][b, :scene["count"][b]])
        assert abs(s - (1 - 0.5 * np.abs(V[a] - V[b]).sum())) <= 1e-12
    for k in range(len(V)):
        c = scene["count"][k]
        # |v|_1 = 1 up to the rounding of the normalisation: c divisions and c adds of numbers below one
        assert abs(oracle.score(scene["word"][k, :c], scene["value"][k, :c], scene["word"][k, :c], scene["value"][k, :c]) - 1) <= 2 * c * 2.0 ** -53
    assert oracle.score([3, 7], [0.25, 0.75], [3, 7], [0.25, 0.75]) == 1.0


def test_a_stamped_unscored_neighbour_adds_its_stale_score():
    """corpus.stale_neighbour: the second query stamps row 3 without scoring it, and row 3 is row 2's covisibility neighbour.  On the
    database that has seen the first query row 3 still holds that query's score (about 0.97), which beats row 2's own (about 0.70):
    the candidate is row 3.  On a fresh database row 3 holds 0 and the candidate is row 2."""
    scene, (q0, q1) = corpus.stale_neighbour()
    db = oracle.Database(scene)
    _, _, id0 = db.detect_n_best(q0, 3)
    w0, s0 = db.device_view(0, id0)
    assert w0[2] == 10 and w0[3] == 10 and 0.9 < s0[3] < 1 and 0.3 < s0[2] < 0.4
    lo1, _, id1 = db.detect_n_best(q1, 3)
    w1, s1 = db.device_view(0, id1)
    assert w1[2] == 11 and w1[3] == 1                              # row 3 is stamped (one common word against eleven) ...
    assert s1[3] == s0[3] and 0.6 < s1[2] < 0.8                    # ... but not scored: it keeps the first query's score
    assert list(lo1) == [3]
    fresh, _, _ = oracle.Database(scene).detect_n_best(q1, 3)
    assert list(fresh) == [2]
    assert list(brute_force(scene, int(q1), s0)["loop"]) == [3] and list(brute_force(scene, int(q1), np.zeros(4, np.float32))["loop"]) == [2]


def test_connected_keyframes_never_appear():
    scene, queries = corpus.base()
    db = oracle.Database(scene)
    seen = 0
    for q in queries:
        lo, me, qid = db.detect_n_best(q, len(scene["count"]))
        conn = set(scene["connected"][int(q)].tolist())
        words, _ = db.device_view(0, qid)
        assert not conn & set(lo.tolist()) and not conn & set(me.tolist()) and not conn & set(db.last_sharing().tolist())
        assert all(words[c] == -1 for c in conn)
        seen += sum(1 for c in conn if scene["db_rank"][c] >= 0 and set(scene["word"][c, :scene["count"][c]]) & set(scene["word"][q, :scene["count"][q]]))
    assert seen >= 10, "connected keyframes in the database that share a word with their query"


def test_math_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "keyframe_database_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "keyframe_database_math_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_adapter_and_call_sites_compile_and_run_against_mocks(tmp_path):
    """include/morb/KeyFrameDatabase.h against the mocks of tests/native/mock_ref and tests/native/mock_keyframe_database: the call
    shapes of LoopClosing.cc:484 and Tracking.cc:3369 compile, and the host side (add / erase / clear / clearMap and the flattening
    of a query) runs, with no GPU call."""
    exe = str(tmp_path / "keyframe_database_call_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_keyframe_database"),
                        "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(NATIVE, "keyframe_database_call_check.cc"),
                        "-L" + os.path.join(ROOT, "morb_slam_amd"), "-lmorb_hip", "-Wl,-rpath," + os.path.join(ROOT, "morb_slam_amd"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "flatten ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_header_declares_and_library_exports_both_entries():
    hdr = open(os.path.join(ROOT, "include", "morb_hip.h")).read()
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    assert os.path.exists(lib), "build() first"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    from morb_slam_amd import ORBmatcher
    from morb_slam_amd.capi import lib as capi_lib
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(morb_matcher\*", hdr) and re.search(r"\bT " + s + r"\b", nm)
        assert getattr(capi_lib(), s).argtypes, s            # derived from the header by cdecl.py
    assert callable(ORBmatcher.DetectNBestCandidates) and callable(ORBmatcher.DetectRelocalizationCandidates)
