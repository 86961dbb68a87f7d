"""The constructed matcher cases (stereo_cases.py, bow_cases.py) checked without a GPU: every case is legal, takes the path or belongs to the
class it claims (through the Python mirror of the kernels' choices), and is not vacuous under the oracle.  The mirror's constants are
compared with the text of csrc/matcher.hip."""
import os
import re

import numpy as np
import pytest

import bow_cases as B
import oracle_lib as O
import stereo_cases as S

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "morb_slam_amd", "csrc", "matcher.hip")


def _constexpr(text, name):
    m = re.search(r"constexpr int [^;]*\b%s = (\d+)\s*[,;]" % name, text)
    assert m, "constexpr int %s not found in matcher.hip" % name
    return int(m.group(1))


def test_mirror_constants_match_the_source():
    text = open(SRC).read()
    for name in ("SM_BAND", "SM_MAXB", "SM_LIST", "SM_KQ", "SM_PCAP", "SMED_V", "TH_LOW", "TH_HIGH", "BM_FJ"):
        assert _constexpr(text, name) == getattr(S, name), "the mirror's %s differs from matcher.hip" % name
    m = re.search(r"inline int sm_lk_for\(int nframes\) \{ return (.*?); \}", text)
    assert m, "sm_lk_for's one-line body not found in matcher.hip"
    steps = tuple((int(a), int(b)) for a, b in re.findall(r"nframes <= (\d+) \? (\d+)", m.group(1)))
    last = int(re.search(r": (\d+)$", m.group(1)).group(1))
    assert (steps, last) == (S.SM_LK_STEPS, S.SM_LK_LAST), "the mirror's sm_lk_for differs from matcher.hip"
    m = re.search(r"if \(nframes <= (\d+)\) hipLaunchKernelGGL\(k_stereo_median<(\d+)>.*\n\s*else hipLaunchKernelGGL\(k_stereo_median<(\d+)>", text)
    assert m, "the two k_stereo_median launches not found in matcher.hip"
    assert tuple(int(g) for g in m.groups()) == (S.SMED_FEW_FRAMES, S.SMED_WAVES_FEW, S.SMED_WAVES_BATCH), "the mirror's SMED_WAVES rule differs from matcher.hip"
    m = re.search(r"__shared__ uint4 tile\[(\d+) \* 2\];", text)
    assert m and int(m.group(1)) == S.KNN2_TILE and "j0 += %d" % S.KNN2_TILE in text, "the mirror's KNN2_TILE differs from matcher.hip"
    assert "n > SM_PCAP - 64" in text and "NL <= NT * SMED_V" in text and "listTotal <= SM_LIST * cap" in text   # the rules themselves
    assert [S.sm_lk_for(n) for n in S.WORKGROUP_SHAPES] == [4, 8, 16, 32]


def test_the_fixture_never_flushes_mid_scan():
    """The finding behind these cases, as a fact: on the extractor's own output for the suite's first stereo pair no wave of any workgroup shape
    collects enough pairs for a mid-scan flush, the band lists stay far below SM_LIST * cap and the median stays in registers."""
    b = S.base()
    c = S._case("fixture", b, {0: S._frame(b, b["kl"], b["dl"], b["kr"], b["dr"])}, cap=1232, nframes=1)
    S.legal(c)
    for nf in S.WORKGROUP_SHAPES:
        p = S.pairs_per_scan(c, 0, nf)
        assert p["mid"] == 0 and p["maxPairs"] <= S.SM_PCAP - 64, (nf, p)
        assert S.median_in_regs(nf, len(b["kl"]))
    assert S.pairs_per_scan(c, 0, 33)["maxPairs"] < 100 and S.pairs_per_scan(c, 0, 1)["maxCand"] < 40
    assert S.use_bands(c, 0) and S.list_total(c, 0) < 2 * c["cap"]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, mk in S.CASES.items():
        c = mk()
        assert S.legal(c), name
        out[name] = (c, {f: S.oracle_matches(c, f) for f in c["frames"]})
    return out


def _matched(cases, name, f=0):
    return int((cases[name][1][f][0] >= 0).sum())


def test_dense_rows_flush_inside_a_run_and_between_keypoints(cases):
    c, ora = cases["dense_row_1"]
    assert c["nframes"] == 1 and S.kq_for(1) == 1 and S.use_bands(c, 0)
    n, best, idx, ties = S.best_candidates(c, 0)
    heavy = [i for _, i in c["classes"]["C"]]
    assert (n[heavy] > S.SM_PCAP).all()                 # more than the list holds: cut by a flush whatever the band's order
    p = S.pairs_per_scan(c, 0)
    assert p["inside"] >= 1 and all(e[2] == 0 for e in p["events"])    # one keypoint per wave: every flush is inside a single run
    assert _matched(cases, "dense_row_1") >= 10

    c, ora = cases["dense_row_8"]
    assert c["nframes"] == 33 and S.kq_for(33) == 8
    fr = c["frames"][0]
    cand = S.candidate_mask(c, 0)
    lists = S._band_lists(c, 0)[0]
    for g, size in (("A", 96), ("B", 100)):
        left = [i for _, i in c["classes"][g]]
        assert [i % 4 for i in left] == [left[0] % 4] * 8 and [i // 4 for i in left] == list(range(8))   # q = 0 .. 7 of one wave of workgroup 0
        band = lists[int(fr["kl"]["y"][left[0]]) // S.SM_BAND]
        assert len(band) == size and cand[np.ix_(left, band)].all()      # every entry a candidate of all eight: 64 + (size - 64) pairs per scan in any order
        assert 60 <= n[left].min() and n[left].max() <= 100
    ev = S.pairs_per_scan(c, 0)["events"]
    assert (0, 0, 4, "between") in ev and (0, 1, 4, "inside") in ev, ev
    # the heavy keypoints exercise the merge: accepted matches whose Hamming winner had ties, and some whose winner is unique
    u = ora[0][0]
    heavy = [i for g in "ABC" for _, i in c["classes"][g]]
    assert sum(u[i] >= 0 and ties[i] > 1 for i in heavy) >= 2 and sum(u[i] >= 0 and ties[i] == 1 for i in heavy) >= 2
    assert _matched(cases, "dense_row_8") >= 10


def test_median_global_leaves_the_registers(cases):
    c, ora = cases["median_global"]
    NL = len(c["frames"][0]["kl"])
    assert c["nframes"] == 17 and not S.median_in_regs(17, NL) and S.median_in_regs(16, NL) and NL <= c["cap"]
    u = ora[0][0]
    assert _matched(cases, "median_global") >= 500
    # the restatement of the SAD distances and of the cut reproduces the oracle's result exactly ...
    md = c["median"]
    acc, dist = md["acc"], md["dist"]
    m, cut = S.median_cut(dist[acc])
    assert m == md["m"]
    exp = acc.copy(); exp[np.nonzero(acc)[0][cut]] = False
    assert ((u >= 0) == exp).all()
    # ... so these are facts about the case: a median one higher would let keypoints through that are cut, and keypoints beyond what the
    # register form holds are among those the cut removes
    th, th1 = np.float32(1.5) * np.float32(1.4) * np.float32(m), np.float32(1.5) * np.float32(1.4) * np.float32(m + 1)
    d32 = dist.astype(np.float32)
    assert (acc & (d32 >= th) & (d32 < th1)).any()
    held = 64 * S.SMED_WAVES_BATCH * S.SMED_V
    assert (acc[held:] & ~exp[held:]).any() and (acc[:held] & ~exp[:held]).any() and exp[held:].any()


def test_unbanded_and_the_band_limit(cases):
    c, _ = cases["unbanded"]
    assert S.list_total(c, 0) > S.SM_LIST * c["cap"] and not S.use_bands(c, 0)
    assert len(c["frames"][0]["kr"]) == c["cap"]
    assert (c["frames"][0]["kr"]["octave"] == 4).sum() > c["cap"] // 2
    assert _matched(cases, "unbanded") >= 10
    c, _ = cases["banded_edge"]
    assert S.list_total(c, 0) == S.SM_LIST * c["cap"] and S.use_bands(c, 0)
    assert S.list_total(c, 1) == S.SM_LIST * c["cap"] + 1 and not S.use_bands(c, 1)
    k0, k1 = c["frames"][0]["kr"], c["frames"][1]["kr"]
    diff = np.nonzero(k0 != k1)[0]
    assert diff.tolist() == [c["classes"]["moved"][0][1]]       # one keypoint moved, across a band border
    assert int(k0["y"][diff[0]]) // S.SM_BAND == int(k1["y"][diff[0]]) // S.SM_BAND and int(k1["y"][diff[0]] + 2) // S.SM_BAND == int(k0["y"][diff[0]]) // S.SM_BAND + 1
    assert _matched(cases, "banded_edge", 0) >= 10 and _matched(cases, "banded_edge", 1) >= 10


def test_threshold_classes(cases):
    c, ora = cases["thresholds"]
    u = ora[0][0]
    n, best, idx, ties = S.best_candidates(c, 0)
    cls = {k: [i for _, i in v] for k, v in c["classes"].items()}
    assert all(len(v) >= 1 for v in cls.values())
    assert (best[cls["best74"]] == 74).all() and (u[cls["best74"]] >= 0).sum() >= 1       # passes the gate (and the SAD stage after it)
    assert (best[cls["best75"]] == 75).all() and (u[cls["best75"]] == -1).all()
    assert (best[cls["best99"]] == 99).all() and (n[cls["best99"]] == 2).all() and (u[cls["best99"]] == -1).all()
    assert (best[cls["only100"]] == 100).all() and (n[cls["only100"]] == 1).all() and (u[cls["only100"]] == -1).all()
    kr = c["frames"][0]["kr"]
    for k in ("tie_low_at_partner", "tie_low_elsewhere", "tie_many"):
        assert (ties[cls[k]] >= 2).all() and (best[cls[k]] < 75).all()
    # which right keypoint won shows in the result: the lower index at the partner's column is refined to a match near it ...
    at = cls["tie_low_at_partner"]
    assert (u[at] >= 0).sum() >= 1 and all(abs(u[i] - kr["x"][idx[i]]) < 8 for i in at if u[i] >= 0)
    # ... and with the lower index 24 px away from the partner the SAD search starts from there (no member ends near the HIGHER index's column)
    for i in cls["tie_low_elsewhere"]:
        assert u[i] < 0 or abs(u[i] - kr["x"][idx[i]]) < 8
    assert (n[cls["tie_many"]] == 130).all() and (u[cls["tie_many"]] >= 0).sum() >= 1
    assert _matched(cases, "thresholds") >= 10


def test_sad_edge_classes(cases):
    c, ora = cases["sad_edges"]
    u, d = ora[0]
    cls = {k: [i for _, i in v] for k, v in c["classes"].items()}
    kl, kr = c["frames"][0]["kl"], c["frames"][0]["kr"]
    n, best, idx, ties = S.best_candidates(c, 0)
    g = [i for v in cls.values() for i in v]
    assert (best[g] == 0).all()                                   # every gadget reaches the SAD stage from its own right keypoint
    assert (idx[g] == np.arange(len(g))).all()
    for i in cls["equal_sad_first"]:
        assert u[i] == kr["x"][idx[i]] - 4                        # zeros at -4, -2, 0, 2, 4: the first wins, deltaR = 0
    for k in ("inc_m5", "inc_p5", "disp_negative"):
        assert (u[cls[k]] == -1).all()
    i = cls["disp_zero"][0]
    assert u[i] == np.float32(np.float64(kl["x"][i]) - 0.01) and d[i] == np.float32(c["mbf"]) / np.float32(0.01)    # the 0.01 branch
    assert _matched(cases, "sad_edges") >= 10


def test_few_matches_classes(cases):
    c, ora = cases["few_matches"]
    for f, want in enumerate((0, 1, 2, 3, 4, 4)):
        u = ora[f][0]
        assert int((u >= 0).sum()) == want and len(c["frames"][f]["kl"]) >= max(want, 1), f
    assert len(c["frames"][0]["kl"]) == 3        # frame 0 has keypoints and candidates; none is accepted: total == 0


def test_geometry_gate_classes(cases):
    c, ora = cases["geometry_gates"]
    u = ora[0][0]
    n, best, idx, ties = S.best_candidates(c, 0)
    cls = {k: [i for _, i in v] for k, v in c["classes"].items()}
    assert set(cls) == set(S.PASSING_GATES) | set(S.FAILING_GATES) and all(len(v) >= 1 for v in cls.values()), {k: len(v) for k, v in cls.items()}
    for k in S.PASSING_GATES:
        assert (n[cls[k]] == 1).all() and (best[cls[k]] < 5).all(), k
    for k in S.FAILING_GATES:
        assert (n[cls[k]] == 0).all() and (u[cls[k]] == -1).all(), k
    kl, kr = c["frames"][0]["kl"], c["frames"][0]["kr"]
    minr, maxr = S._right_rows(c, kr)
    row = kl["y"].astype(np.int64)
    for i in cls["minr_in"]: assert row[i] == minr[i]
    for i in cls["minr_out"]: assert row[i] == minr[i] - 1
    for i in cls["maxr_in"]: assert row[i] == maxr[i]
    for i in cls["maxr_out"]: assert row[i] == maxr[i] + 1
    maxD = np.float32(c["mbf"]) / np.float32(c["mb"])
    for i in cls["xr_eq_ul"]: assert kr["x"][i] == kl["x"][i]
    for i in cls["xmin_eq"]: assert kr["x"][i] == np.float32(kl["x"][i] - maxD)
    assert kl["y"][cls["row19"][0]] == 19 and kl["y"][cls["row_hm20"][0]] == c["size"][1] - 20
    for k, dO in (("oct_m1", -1), ("oct_p1", 1), ("oct_m2", -2), ("oct_p2", 2)):
        assert all(kr["octave"][i] - kl["octave"][i] == dO for i in cls[k])
    passed = [i for k in S.PASSING_GATES for i in cls[k]]
    assert (u[passed] >= 0).sum() >= 10         # the passing gates lead to real matches


# ---- the BoW corpus ----
@pytest.fixture(scope="module")
def corpus():
    return B.corpus()


def _bow(c, p, ratio, ori, nLeft=None):
    kf, fr = c["pairs"][p]
    a, b = c["images"][kf], c["images"][fr]
    if nLeft is None:
        return O.search_by_bow(a["desc"], a["angle"], a["has"], a["node"], b["desc"], b["angle"], b["node"], ratio, ori)
    return O.search_by_bow_fisheye(a["desc"], a["angle"], a["has"], a["node"], b["desc"], b["angle"], b["node"], nLeft, ratio, ori)


def test_bow_corpus_layout(corpus):
    c = corpus
    assert c["cap"] % 64 != 0 and c["images"][1]["count"] == c["cap"] and c["images"][3]["count"] == 0 and c["images"][4]["count"] == 1
    assert (0, 0) in c["pairs"]
    K, F = c["images"][0], c["images"][1]
    sizes = lambda im: {int(n): int(k) for n, k in zip(*np.unique(im["node"][im["node"] >= 0], return_counts=True))}
    sk, sf = sizes(K), sizes(F)
    assert set(B.FRAME_NODE_SIZES) <= set(sf.values()) and set(B.KF_NODE_SIZES) <= set(sk.values())
    assert set(sk) - set(sf) and set(sf) - set(sk) and (K["node"] == -1).any() and (F["node"] == -1).any()
    assert (1 << 20) in sk and 0x7fffffff in sk and 0 in sk
    big = [n for n, k in sf.items() if k >= S.BM_FJ * 64]
    assert len(big) == 2 and all(n in sk for n in big)           # 256 and 257 frame features: the general path, with keyframe features to match
    for n in big:                                                # ... interleaved with other nodes' features in index order
        i = np.nonzero(F["node"] == n)[0]
        assert (np.diff(i) > 1).any()


@pytest.mark.parametrize("ratio", B.RATIOS)
def test_bow_classes(corpus, ratio):
    c = corpus
    res = {}
    seen = set()
    for name, items in c["classes"].items():
        for p, side, index, expected in items:
            if p not in res:
                res[p] = (_bow(c, p, ratio, True), _bow(c, p, ratio, False)) if p != c["fish_pair"] else \
                    (_bow(c, p, ratio, True, c["nLeft"][p][0]),) * 2
            (n1, m1), (n0, m0) = res[p]
            if side == "N":
                assert (n0, n1) == (index, expected), (name, n0, n1)
            elif name.startswith("ratio_") and not name.endswith("_%g" % ratio):
                continue
            else:
                assert m1[index] == expected, (name, ratio, index, int(m1[index]), expected)
            seen.add(name)
    want = {"best50", "best51", "best49", "tie_fails", "tie_last_left", "node_sparse", "node_max", "node_zero", "no_word", "greedy_chunk",
            "greedy_slot", "hist_tied_tops", "hist_at_tenth", "hist_below_tenth", "hist_third_below", "rounding", "right50", "right51",
            "right_tie", "right_needs_left"} | {"ratio_%s_%g" % (k, ratio) for k in ("below", "equal", "above")}
    assert want <= seen, want - seen
    # not vacuous: the size ladder matches under every form
    assert res[0][0][0] >= 40
    a, b = c["images"][0], c["images"][1]
    n, m = O.search_by_bow_kfkf(a["desc"], a["angle"], a["has"], a["node"], c["nValid"][0], b["desc"], b["angle"], b["has"], b["node"], c["nValid"][1],
                                ratio, True)
    assert n >= 10 and 0 < c["nValid"][0] < a["count"] and 0 < c["nValid"][1] < b["count"]
    # the strict threshold of the keyframe form: 49 matches, 50 does not
    cls = c["classes"]
    n, m = O.search_by_bow_kfkf(a["desc"], a["angle"], a["has"], a["node"], a["count"], b["desc"], b["angle"], b["has"], b["node"], b["count"], ratio, True)
    assert m[cls["best49"][0][3]] == cls["best49"][0][2] and m[cls["best50"][0][3]] == -1
    # nValid cuts node segments on either side
    for im, nv in ((a, c["nValid"][0]), (b, c["nValid"][1])):
        assert any((im["node"][:nv] == nd).any() and (im["node"][nv:im["count"]] == nd).any() for nd in np.unique(im["node"][im["node"] >= 0]))
    # fisheye on the main pair: Nleft inside a node's segment changes the result
    n_mid, m_mid = _bow(c, 0, ratio, True, c["nLeft"][0][2])
    assert n_mid != res[0][0][0] or (m_mid != res[0][0][1]).any()


def test_knn2_and_vocabulary_inputs():
    probs = B.knn2_problems()
    assert sorted({len(t) - to for q, t, qo, to in probs}) == [1, 255, 256, 257, 512, 513]
    assert sorted({len(q) - qo for q, t, qo, to in probs}) == [1, 255, 256, 257]
    assert any(qo for _, _, qo, _ in probs) and any(to for _, _, _, to in probs)
    dup = 0
    for q, t, qo, to in probs:
        idx, dist = O.knn2(q[qo:], t[to:])
        assert dist[0, 0] == 0                                   # the query equal to a train row
        both = (idx[:, 1] >= 0) & (dist[:, 0] == dist[:, 1])
        assert (idx[both, 0] < idx[both, 1]).all()
        dup += int(both.sum())
    assert dup >= 10                                             # duplicated train descriptors really are best and second best
    vd, vf, feats = B.duplicated_vocabulary()
    w, nd = O.bow_transform(feats, vd, vf, 6, 3, 1)
    first = {int(vf[n]) + 1 for n in np.nonzero(vf >= 0)[0]} | {int(vf[n]) + 2 for n in np.nonzero(vf >= 0)[0]}
    second = {int(vf[n]) + 3 for n in np.nonzero(vf >= 0)[0]} | {int(vf[n]) + 5 for n in np.nonzero(vf >= 0)[0]}
    assert len(set(w.tolist()) & first) >= 10 and not set(w.tolist()) & second and not set(nd.tolist()) & second
