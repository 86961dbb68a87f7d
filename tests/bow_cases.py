"""Constructed node tables and descriptors for the three SearchByBoW forms of k_bow_match (csrc/matcher.hip), and inputs for k_knn2 and
k_bow_transform.  No images: a corpus is a pool of feature sets (descriptor, angle, node id, hasMP per feature, a count per image) with one
capacity, and the list of (keyframe image, frame image) pairs to search.

Inside a node every descriptor is a thermometer code on one line: feature at position p has its p lowest bits set (p < 192), so two
features of a node are exactly |p1 - p2| apart; the top 64 bits carry a per-node signature so that features of different nodes are not
mistaken for each other unnoticed.  A node is therefore a list of keyframe positions and a list of frame positions, visited in index order:
the reference's greedy loop, its thresholds and its ratio test can be aimed at exactly.

Index order: an image's features are dealt round-robin over its nodes (rank inside the node first, node second), so every node's features
are interleaved with all others' while keeping their order inside the node; features flagged `right` (the right camera of a fisheye frame)
follow all the others.  Images are padded with node -1 features (no word) up to the wanted count.

Classes: corpus["classes"][name] = [(pair, side, index, expected)].  Side "F": frame feature `index` of the pair must end matched to the
keyframe feature `expected` (-1: unmatched) in the keyframe-to-frame form (a class named ratio_*_<r> at ratio r, every other at every ratio).
Side "N": the pair holds `index` matches before the orientation filter and `expected` after it. test_matcher_cases_cpu.py checks every entry against the oracle,
so that a class that does not do what its name says is a failure there, not on the GPU."""
import numpy as np

from stereo_cases import BM_FJ, KNN2_TILE, TH_LOW, thermo_low

RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)
FRAME_NODE_SIZES = (1, 63, 64, 65, 128, 192, 255, 256, 257)     # BM_FJ * 64 = 256 is the first size on the general path
KF_NODE_SIZES = (1, 64, 65, 128, 129)
assert BM_FJ * 64 == 256 and TH_LOW == 50 and KNN2_TILE == 256


def desc_at(pos, sig):
    d = thermo_low(int(pos)).copy()
    d[24:] = sig
    return d


class Image:
    def __init__(self, seed):
        self.f = []          # (node, pos, angle, has, right)
        self.rng = np.random.default_rng(seed)

    def add(self, node, pos, angle=0.0, has=1, right=False):
        self.f.append([node, pos, angle, has, right]); return len(self.f) - 1

    def build(self, count=None):
        """-> dict(desc, angle, node, has, count, index: handle -> final index)."""
        rank, seen, order = [], {}, {}
        for h, (node, *_r) in enumerate(self.f):
            order.setdefault(node, len(order))
            rank.append(seen.get(node, 0)); seen[node] = rank[-1] + 1
        hs = sorted(range(len(self.f)), key=lambda h: (self.f[h][4], rank[h], order[self.f[h][0]]))
        n = len(hs) if count is None else count
        assert n >= len(hs)
        sigs = {}
        desc = np.zeros((n, 32), np.uint8); angle = np.zeros(n, np.float32); node = np.full(n, -1, np.int32); has = np.ones(n, np.uint8)
        index = {}
        for i, h in enumerate(hs):
            nd, pos, ang, hm, _ = self.f[h]
            if nd not in sigs:
                sigs[nd] = np.random.default_rng(abs(int(nd)) % (2 ** 31) + 17).integers(0, 256, 8, dtype=np.uint8)
            desc[i], angle[i], node[i], has[i] = desc_at(pos, sigs[nd]), ang, nd, hm
            index[h] = i
        desc[len(hs):] = self.rng.integers(0, 256, (n - len(hs), 32), dtype=np.uint8)     # no word: never looked at
        nleft = sum(1 for h in hs if not self.f[h][4])
        return dict(desc=desc, angle=angle, node=node, has=has, count=n, index=index, nleft=nleft)


def ratio_equalities():
    """Per ratio r: (d1, d2) with float32(d1) == float32(r) * float32(d2) exactly as the kernel and the reference compute it, d1 <= TH_LOW."""
    out = {}
    for r in RATIOS:
        rf = np.float32(r)
        out[r] = [(d1, d2) for d2 in range(2, 192) for d1 in range(1, TH_LOW) if np.float32(d1) == rf * np.float32(d2)]
        assert out[r], r
    return out


def main_pair(classes, pair=0):
    """The keyframe / frame pair that holds the node layout and the decisions at equality (all angles 0: one histogram bin)."""
    K, F = Image(1), Image(2)
    exp = []     # (class, frame handle, keyframe handle or None)
    nid = [100]

    def node():
        nid[0] += 7; return nid[0]

    def simple(cls, fpos, kpos=(0,), expect=None, nd=None):
        """one node; expect = [(frame position index, keyframe position index or None)]"""
        nd = node() if nd is None else nd
        kh = [K.add(nd, p) for p in kpos]; fh = [F.add(nd, p) for p in fpos]
        for fi, ki in expect or []:
            exp.append((cls, fh[fi], None if ki is None else kh[ki]))
        return kh, fh
    # thresholds of the keyframe-to-frame form (<= TH_LOW) and of the keyframe-to-keyframe form (< TH_LOW)
    simple("best50", (50, 180), expect=[(0, 0)]); simple("best51", (51, 180), expect=[(0, None)])
    simple("best49", (49, 180), expect=[(0, 0)])
    # the float ratio test at equality and one either side, for every ratio (a node aimed at one ratio is ordinary data for the others)
    for r, eqs in ratio_equalities().items():
        d1, d2 = eqs[len(eqs) // 2]
        for cls, d in (("ratio_below", d1 - 1), ("ratio_equal", d1), ("ratio_above", d1 + 1)):     # (expected AT ratio r)
            simple("%s_%g" % (cls, r), (d, d2), expect=[(0, 0 if cls == "ratio_below" else None)])
    # a tie at the best distance fails the ratio test ...
    simple("tie_fails", (20, 20), expect=[(0, None), (1, None)])
    # ... except when the tied candidate is the last one left: q0 at 100 takes s0 at 110; q1 at 135 is 25 from s0 and from s1 at 160
    simple("tie_last_left", (110, 160), kpos=(100, 135), expect=[(0, 0), (1, 1)])
    # node ids: sparse and large, a node on one side only, no word
    simple("node_sparse", (3,), nd=1 << 20, expect=[(0, 0)]); simple("node_max", (4,), nd=0x7fffffff, expect=[(0, 0)])
    simple("node_zero", (5,), nd=0, expect=[(0, 0)])
    K.add(node(), 7); F.add(node(), 7)                       # two nodes, each on one side only
    simple("no_word", (0,), nd=-1, expect=[(0, None)])       # node id -1 on both sides: equal descriptors, never compared
    # the size ladder: keyframe features with and without a MapPoint, positions at random on the line — the oracle decides; the sizes aim
    # at the register slots (64 per slot), the general path (256 and up) and the keyframe chunks of 64
    rng = np.random.default_rng(3)
    for nf, nk in zip(FRAME_NODE_SIZES, (1, 64, 65, 128, 129, 1, 64, 65, 129)):
        nd = node()
        for p in rng.integers(0, 192, nk): K.add(nd, p, has=int(rng.random() < 0.8))
        for p in rng.integers(0, 192, nf): F.add(nd, p, has=int(rng.random() < 0.8))
    # the greedy dependency: q wants what q - 1 just took.  Across a keyframe chunk boundary: a keyframe node of 70, positions 63 and 64 the
    # pair (at 100 and 104), the others without a MapPoint; the frame's s0 at 102 is 2 from both, s1 at 140 is what q = 64 must settle for.
    nd = node()
    kh = [K.add(nd, 100 if q == 63 else 104 if q == 64 else 0, has=int(q in (63, 64))) for q in range(70)]
    fh = [F.add(nd, 102), F.add(nd, 140)]
    exp += [("greedy_chunk", fh[0], kh[63]), ("greedy_chunk", fh[1], kh[64])]
    # across register slots of the frame side: a frame node of 130; s at rank 10 (slot 0, position 102) is the contested one, s at rank 70
    # (slot 1, position 120) and at rank 129 (slot 2, position 150) the fall-backs of the second and third keyframe feature; every other frame
    # feature far away (position 0)
    nd = node()
    kh = [K.add(nd, 100), K.add(nd, 104), K.add(nd, 108)]
    fh = [F.add(nd, {10: 102, 70: 120, 129: 150}.get(s, 0)) for s in range(130)]
    exp += [("greedy_slot", fh[10], kh[0]), ("greedy_slot", fh[70], kh[1]), ("greedy_slot", fh[129], kh[2])]
    for cls, f_, k_ in exp:
        classes.setdefault(cls, []).append([pair, "F", ("h", f_), ("h", k_)])
    return K, F


def histogram_pair(bins, seed):
    """A pair whose matches are exact copies (distance 0, one node each) with rot = 30 * bin + 3 degrees: `bins` = [(bin, matches)]."""
    K, F = Image(seed), Image(seed + 1)
    nd = 1000
    for b, n in bins:
        for _ in range(n):
            nd += 1
            K.add(nd, 9, angle=30.0 * b + 3.0); F.add(nd, 9, angle=0.0)
    return K, F


def rounding_pair():
    """Angle differences on a bin border: 15 (0.5 -> bin 1), 45 (1.5 -> 2) and 345 degrees (11.5 -> 12), negative differences that wrap
    (10 - 350 -> 20 -> bin 1; 0.5 - 15.5 -> 345 -> bin 12), just under 360 (bin 12), and two matches at 150 (bin 5) that the histogram drops:
    bins 1 and 12 hold four matches, bin 2 three."""
    K, F = Image(40), Image(41)
    nd = 2000
    for ak, af in [(15.0, 0.0)] * 3 + [(45.0, 0.0)] * 3 + [(345.0, 0.0)] * 2 + [(10.0, 350.0), (0.5, 15.5), (359.99, 0.0), (150.0, 0.0), (200.0, 50.0)]:
        nd += 1
        K.add(nd, 9, angle=ak); F.add(nd, 9, angle=af)
    return K, F


def fisheye_pair(classes, pair):
    """The right camera's side of the fisheye form: its features are ranked apart, without a ratio test, and only when the LEFT best passes
    TH_LOW.  Per node one keyframe feature at 0 and a left frame feature at 10 (the left match), then on the right:
      right50 / right51      the right best at 50 (taken) and at 51 (not taken)
      right_tie              two right features at 20: the lower index wins (no ratio test on that side)
      right_needs_left       no left feature at all: the right best at 5 is never looked at"""
    K, F = Image(50), Image(51)
    nd = 3000
    for cls, left, right, want in (("right50", (10, 150), (50,), 0), ("right51", (10, 150), (51,), None), ("right_tie", (10, 150), (20, 20), 0),
                                   ("right_needs_left", (), (5,), None)):
        nd += 1
        kh = K.add(nd, 0)
        for p in left: F.add(nd, p)
        rh = [F.add(nd, p, right=True) for p in right]
        classes.setdefault(cls, []).append([pair, "F", ("h", rh[0]), ("h", kh if want is not None else None)])
        if cls == "right_tie":
            classes[cls].append([pair, "F", ("h", rh[1]), ("h", None)])
    return K, F


HIST_KEPT = dict(hist_tied_tops=15, hist_at_tenth=24, hist_below_tenth=20, hist_third_below=22)


def corpus():
    """-> dict(cap, images [dict], pairs [(kf image, frame image)], nLeft {pair: F.Nleft}, nValid [per image], classes, fisheye_pairs,
    kfkf_nvalid).  Image 0 / 1: the main pair (image 1 padded to count == cap, a capacity that is no multiple of 64); 2: image 1 with no
    MapPoint at all; 3: empty; 4: one feature; then the histogram, rounding and fisheye pairs."""
    classes = {}
    K, F = main_pair(classes)
    imgs = [K, F]
    n1 = len(F.f)
    cap = n1 + 37 if (n1 + 37) % 64 else n1 + 38
    built = [K.build(), F.build(count=cap)]
    noMP = dict(built[1]); noMP["has"] = np.zeros_like(built[1]["has"]); built.append(noMP)
    built.append(Image(9).build())                     # count 0
    one = Image(10); one.add(0, 5); built.append(one.build())   # count 1: node 0, 0 away from the main pair's node-0 features
    pairs = [(0, 1), (0, 0), (1, 0), (0, 3), (3, 0), (4, 0), (0, 4), (0, 2)]
    hist = {"hist_tied_tops": [(2, 5), (4, 5), (6, 5), (8, 5)],              # the first three stay
            "hist_at_tenth": [(3, 20), (5, 2), (7, 2), (9, 1)],              # max2 == max3 == 0.1f * max1: both stay; bin 9 goes
            "hist_below_tenth": [(3, 20), (5, 1), (7, 1)],                   # one below: both go
            "hist_third_below": [(3, 20), (5, 2), (7, 1)]}                   # max3 one below: only it goes
    for n, (name, bins) in enumerate(hist.items()):
        a, b = histogram_pair(bins, 20 + 2 * n)
        built += [a.build(), b.build()]; pairs.append((len(built) - 2, len(built) - 1))
        classes[name] = [[len(pairs) - 1, "N", sum(n for _, n in bins), HIST_KEPT[name]]]
    a, b = rounding_pair()
    built += [a.build(), b.build()]; pairs.append((len(built) - 2, len(built) - 1))
    classes["rounding"] = [[len(pairs) - 1, "N", 13, 11]]
    a, b = fisheye_pair(classes, len(pairs))
    built += [a.build(), b.build()]; pairs.append((len(built) - 2, len(built) - 1))
    fish_pair = len(pairs) - 1
    # handles -> final indices
    for cls, items in classes.items():
        for it in items:
            if it[1] == "F":
                kf, fr = pairs[it[0]]
                it[2] = built[fr]["index"][it[2][1]]
                it[3] = -1 if it[3][1] is None else built[kf]["index"][it[3][1]]
    assert all(b["count"] <= cap for b in built)
    n1 = built[1]["count"]
    nLeft = {0: [0, n1, n1 // 3, -1], fish_pair: [built[pairs[fish_pair][1]]["nleft"]]}     # F.Nleft values to run a pair at (-1: pinhole)
    nValid = [b["count"] for b in built]
    nValid[0], nValid[1] = built[0]["count"] // 2, (2 * built[1]["count"]) // 3               # cut node segments on either side
    return dict(cap=cap, images=built, pairs=pairs, nLeft=nLeft, nValid=nValid, classes=classes, fish_pair=fish_pair)


def pool_arrays(c):
    """The corpus as the [nimg, cap, ...] host arrays the C entry points take: (kps records with the angle field, desc, node, has, count)."""
    from oracle_lib import KP_DTYPE
    nimg, cap = len(c["images"]), c["cap"]
    kps = np.zeros((nimg, cap), KP_DTYPE); desc = np.zeros((nimg, cap, 32), np.uint8)
    node = np.full((nimg, cap), -1, np.int32); has = np.zeros((nimg, cap), np.uint8); cnt = np.zeros(nimg, np.int32)
    rng = np.random.default_rng(77)
    for i, b in enumerate(c["images"]):
        n = b["count"]
        kps[i, :n]["angle"] = b["angle"]; desc[i, :n] = b["desc"]; node[i, :n] = b["node"]; has[i, :n] = b["has"]; cnt[i] = n
        # rows at and beyond the count hold what a real pool would: stale features with words and MapPoints, which must never match
        desc[i, n:] = rng.integers(0, 256, (cap - n, 32), dtype=np.uint8); node[i, n:] = 0; has[i, n:] = 1
    return kps, desc, node, has, cnt


# ---- k_knn2 ----
def knn2_problems():
    """Problems (query [nq, 32], train [nt, 32], query offset, train offset) at the train tile's edges (256 per tile) and the query block's
    (256 per workgroup): train counts 1, 255, 256, 257, 512, 513 and query counts 1, 255, 256, 257 after the offsets.  Train sets hold
    duplicated descriptors (the lower index must come first, as best and as second best), and query 0 equals a train row."""
    rng = np.random.default_rng(8)
    out = []
    for n, (nq, nt, qo, to) in enumerate(((1, 1, 0, 0), (255, 255, 3, 0), (256, 256, 0, 5), (257, 257, 2, 7), (1, 512, 0, 0), (256, 513, 1, 1),
                                          (257, 1, 0, 300), (255, 512, 260, 256))):
        t = rng.integers(0, 256, (nt + to, 32), dtype=np.uint8)
        q = rng.integers(0, 256, (nq + qo, 32), dtype=np.uint8)
        if nt >= 2:
            for a in range(0, nt - 1, 37):           # duplicates inside the searched range, some across a tile edge
                t[to + min(a + 29 + (a % 5) * 60, nt - 1)] = t[to + a]
            k = min(nq, nt)
            q[qo + 1:qo + k:3] = t[to + 1:to + k:3] ^ np.packbits(rng.random((len(range(1, k, 3)), 256)) < 0.05, axis=1)   # near copies: close best matches
        q[qo] = t[to + nt - 1]                        # a query equal to a train row (the last: behind its duplicates, if any)
        out.append((q, t, qo, to))
    return out


# ---- k_bow_transform ----
def duplicated_vocabulary(k=6, L=3, seed=3):
    """A complete k-ary vocabulary in which, under every inner node, child 3 repeats child 1 and child 5 repeats child 2: a feature closest to a
    repeated descriptor must descend into the FIRST of the two.  Returns (nodeDesc, firstChild, features [n, 32]): the features are noisy
    copies of node descriptors of every level, so that many of them are closest to a repeated child."""
    from morb_slam_amd.synth import make_vocabulary
    vd, vf = make_vocabulary(k, L, seed=seed)
    vd = vd.copy()
    for n in np.nonzero(vf >= 0)[0]:
        c0 = vf[n]
        vd[c0 + 3] = vd[c0 + 1]; vd[c0 + 5] = vd[c0 + 2]
    rng = np.random.default_rng(seed)
    src = rng.integers(1, len(vd), 400)
    feats = vd[src] ^ np.packbits(rng.random((400, 256)) < 0.04, axis=1)
    return vd, vf, feats
