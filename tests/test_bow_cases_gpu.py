"""SearchByBoW (keyframe to frame, keyframe to keyframe, fisheye), knn2 and the DBoW2 transform on the constructed inputs of bow_cases.py:
node sizes at the register / general-path and chunk boundaries of k_bow_match, decisions at equality, histogram ties, the train tiles of
k_knn2, duplicated sibling descriptors in k_bow_transform.  Match tables and counts bit for bit against the oracle; what each class of the
corpus does under the oracle is asserted in test_matcher_cases_cpu.py."""
import numpy as np
import pytest

import bow_cases as B
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    import torch
    c = B.corpus()
    kps, desc, node, has, cnt = B.pool_arrays(c)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(kps=dev(kps.view(np.uint8).reshape(kps.shape + (28,))), desc=dev(desc), node=dev(node), has=dev(has), cnt=dev(cnt),
             kf=torch.tensor([p[0] for p in c["pairs"]], dtype=torch.int32, device="cuda"),
             fr=torch.tensor([p[1] for p in c["pairs"]], dtype=torch.int32, device="cuda"))
    return c, t


def _img(c, i):
    b = c["images"][i]
    return b["desc"], b["angle"], b["has"], b["node"], b["count"]


@pytest.mark.parametrize("ratio", B.RATIOS)
@pytest.mark.parametrize("ori", [True, False])
def test_search_by_bow(pool, ratio, ori):
    import torch
    from morb_slam_amd import ORBmatcher
    c, t = pool
    m = ORBmatcher(ratio, ori)
    match, nm = m.SearchByBoW(t["kf"], t["fr"], t["kps"], t["desc"], t["node"], t["cnt"], t["has"])
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, (a, b) in enumerate(c["pairs"]):
        dA, aA, hA, nA, _ = _img(c, a); dB, aB, _, nB, cB = _img(c, b)
        ne, me = O.search_by_bow(dA, aA, hA, nA, dB, aB, nB, ratio, ori)
        assert nm[p] == ne, (p, int(nm[p]), ne)
        np.testing.assert_array_equal(match[p, :cB], me[:cB], err_msg="pair %d" % p)
        assert (match[p, cB:] == -1).all()
        tot += ne
    assert tot >= 100


@pytest.mark.parametrize("ratio", B.RATIOS)
@pytest.mark.parametrize("ori", [True, False])
def test_search_by_bow_keyframes(pool, ratio, ori):
    """The strict threshold, hasMP on both sides, vbMatched2 (the general path keeps it in global memory: the 256- and 257-feature nodes), nValid
    cutting node segments of both keyframes, and a second keyframe without any MapPoint."""
    import torch
    from morb_slam_amd import ORBmatcher
    c, t = pool
    m = ORBmatcher(ratio, ori)
    for nValid in (c["nValid"], [b["count"] for b in c["images"]]):
        nv = torch.tensor(nValid, dtype=torch.int32, device="cuda")
        m12, nm = m.SearchByBoWKeyFrames(t["kf"], t["fr"], t["kps"], t["desc"], t["node"], t["cnt"], t["has"], nValid=nv)
        torch.cuda.synchronize()
        m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
        tot = 0
        for p, (a, b) in enumerate(c["pairs"]):
            dA, aA, hA, nA, cA = _img(c, a); dB, aB, hB, nB, _ = _img(c, b)
            ne, me = O.search_by_bow_kfkf(dA, aA, hA, nA, nValid[a], dB, aB, hB, nB, nValid[b], ratio, ori)
            assert nm[p] == ne, (p, int(nm[p]), ne)
            np.testing.assert_array_equal(m12[p, :cA], me[:cA], err_msg="pair %d" % p)
            assert (m12[p, cA:] == -1).all()
            if (a, b) == (0, 2):
                assert ne == 0              # hasMP2 all zero
            tot += ne
        assert tot >= 50


@pytest.mark.parametrize("ratio", [0.6, 0.75, 0.9])
@pytest.mark.parametrize("ori", [True, False])
def test_search_by_bow_fisheye(pool, ratio, ori):
    """F.Nleft = 0, the count, inside a node's segment and -1 (pinhole through the fisheye entry) on the main pair; the right camera's own
    best at 50 / 51, its ties and its dependence on the left best on the fisheye pair."""
    import torch
    from morb_slam_amd import ORBmatcher
    c, t = pool
    m = ORBmatcher(ratio, ori)
    runs = [(p, nl) for p, nls in c["nLeft"].items() for nl in nls]
    kf = torch.tensor([c["pairs"][p][0] for p, _ in runs], dtype=torch.int32, device="cuda")
    fr = torch.tensor([c["pairs"][p][1] for p, _ in runs], dtype=torch.int32, device="cuda")
    nl = torch.tensor([n for _, n in runs], dtype=torch.int32, device="cuda")
    match, nm = m.SearchByBoW(kf, fr, t["kps"], t["desc"], t["node"], t["cnt"], t["has"], nLeft=nl)
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    res = []
    for r, (p, n) in enumerate(runs):
        a, b = c["pairs"][p]
        dA, aA, hA, nA, _ = _img(c, a); dB, aB, _, nB, cB = _img(c, b)
        ne, me = O.search_by_bow_fisheye(dA, aA, hA, nA, dB, aB, nB, n, ratio, ori)
        assert nm[r] == ne, (p, n, int(nm[r]), ne)
        np.testing.assert_array_equal(match[r, :cB], me[:cB], err_msg="pair %d nLeft %d" % (p, n))
        res.append(ne)
    assert len(set(res[:4])) >= 2 and res[-1] >= 5     # Nleft changes what the main pair matches; the fisheye pair matches on both sides


def test_knn2_tiles():
    import torch
    from morb_slam_amd import ORBmatcher
    probs = B.knn2_problems()
    qp = max(len(q) for q, _, _, _ in probs) + 3; tp = max(len(t) for _, t, _, _ in probs) + 5
    rng = np.random.default_rng(1)
    Q = rng.integers(0, 256, (len(probs), qp, 32), dtype=np.uint8); T = rng.integers(0, 256, (len(probs), tp, 32), dtype=np.uint8)   # stale rows beyond the counts
    for i, (q, t, _, _) in enumerate(probs):
        Q[i, :len(q)] = q; T[i, :len(t)] = t
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    idx, dist = ORBmatcher().knn2(torch.from_numpy(Q).cuda(), i32([len(q) for q, _, _, _ in probs]), torch.from_numpy(T).cuda(),
                                  i32([len(t) for _, t, _, _ in probs]), i32([qo for _, _, qo, _ in probs]), i32([to for _, _, _, to in probs]))
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for i, (q, t, qo, to) in enumerate(probs):
        ie, de = O.knn2(q[qo:], t[to:])
        n = len(q) - qo
        np.testing.assert_array_equal(idx[i, :n], ie, err_msg="problem %d" % i)
        np.testing.assert_array_equal(dist[i, :n], de, err_msg="problem %d" % i)
        assert (idx[i, n:] == -1).all() and (dist[i, n:] == -1).all()


def test_bow_transform_first_of_equal_children():
    import torch
    from morb_slam_amd import ORBmatcher
    vd, vf, feats = B.duplicated_vocabulary()
    counts = [1, 63, 65, 130, 400, 0]
    cap = 401
    desc = np.random.default_rng(2).integers(0, 256, (len(counts), cap, 32), dtype=np.uint8)
    for i, n in enumerate(counts):
        desc[i, :n] = feats[(np.arange(n) * 7 + i) % len(feats)]
    m = ORBmatcher()
    for lup in (1, 2, 3):
        w, nd = m.bow_transform(torch.from_numpy(desc).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"),
                                torch.from_numpy(vd).cuda(), torch.from_numpy(vf).cuda(), 6, 3, lup)
        torch.cuda.synchronize()
        w, nd = w.cpu().numpy(), nd.cpu().numpy()
        for i, n in enumerate(counts):
            we, ne = O.bow_transform(desc[i, :n], vd, vf, 6, 3, lup)
            np.testing.assert_array_equal(w[i, :n], we[:n]); np.testing.assert_array_equal(nd[i, :n], ne[:n])
            assert (w[i, n:] == -1).all() and (nd[i, n:] == -1).all()
