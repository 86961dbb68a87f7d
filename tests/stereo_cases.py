"""Constructed inputs for ComputeStereoMatches (k_stereo_prep / k_stereo_match / k_stereo_median of csrc/matcher.hip): keypoint sets that
reach the branches the extractor's own output never reaches, their legality check, and a Python mirror of the kernels' path choices
(test_matcher_cases_cpu.py pins the mirror's constants against the source text and asserts each case's path; test_stereo_cases_gpu.py runs
the cases).  The convention is that of search_tiers.py: a test says through the mirror which path it means to run before it runs it.

A case is a dict:
  name, size (w, h), ext (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST), mbf, mb, cap, nframes,
  frames {frame index: dict(imgL, imgR, kl, dl, kr, dr)}   keypoints KP_DTYPE, descriptors u8 [n, 32]; count = len
  classes {class name: [(frame, left index), ...]}          the left keypoints built for a named decision
Frames that `frames` does not list have count 0 on both sides (and the images of the first listed frame): they pad the batch to the frame
count a workgroup shape needs and cost nothing on the oracle side.  with_nframes(case, n) gives the same case in a batch of n frames.

LEGALITY.  The stored pyramid border is 3 pixels; pyramid_layout.h (pyr_stereo_extent, pyr_stereo_scale_ok) proves the SAD reads stay inside
stored pixels only for keypoints the extractor itself could emit.  legal(case) asserts exactly that and every test calls it first.

What the kernels decide and the mirror restates:
  k_stereo_match   workgroup = sm_lk_for(nframes) left keypoints, wave wv's keypoint q is iL0 + 4 q + wv; the wave appends (q, iR) pairs
                   of all its keypoints to one list and compares ("flushes") it when the scans end, or mid-scan once it holds more than
                   SM_PCAP - 64 pairs after a 64-entry step; a run cut by a flush meets its own earlier minimum in bestL[q].
                   The scan walks the keypoint's 16-row band list when listTotal <= SM_LIST * cap, else all right keypoints.
  k_stereo_median  reads the SAD distances into registers when NL <= 64 * SMED_WAVES * SMED_V, else from global memory.
The order of a band's list is the order in which k_stereo_prep's LDS atomics arrive, so it is not a function of the inputs.  The mirror
walks a band in ascending right index; the dense cases are built so that what they claim holds for every order (see dense_rows)."""
import functools
import hashlib

import numpy as np

import oracle_lib as O
from oracle_lib import KP_DTYPE

EDGE = 19

# ---- the mirror's constants (test_matcher_cases_cpu.py::test_mirror_constants_match_the_source) ----
SM_BAND, SM_MAXB, SM_LIST, SM_KQ, SM_PCAP = 16, 256, 4, 8, 512
SMED_V = 8
SMED_WAVES_FEW, SMED_WAVES_BATCH, SMED_FEW_FRAMES = 16, 4, 16   # k_stereo_median<16> for nframes <= 16, <4> beyond
SM_LK_STEPS, SM_LK_LAST = ((2, 4), (8, 8), (32, 16)), 32         # sm_lk_for: nframes <= 2 ? 4 : nframes <= 8 ? 8 : nframes <= 32 ? 16 : 32
TH_LOW, TH_HIGH = 50, 100
BM_FJ = 4          # k_bow_match: frame features of a node per lane in registers; BM_FJ * 64 is the first size on the general path
KNN2_TILE = 256    # k_knn2: train descriptors per LDS tile

DEFAULT_EXT = (1200, 1.2, 8, 20, 7)
EUROC = (np.float32(458.654 * 0.11), np.float32(0.11))   # mbf, mb
WORKGROUP_SHAPES = (1, 3, 9, 33)                          # frame counts with SM_LK = 4, 8, 16, 32


def sm_lk_for(nframes):
    for lim, lk in SM_LK_STEPS:
        if nframes <= lim:
            return lk
    return SM_LK_LAST


def kq_for(nframes):
    assert sm_lk_for(nframes) // 4 <= SM_KQ
    return sm_lk_for(nframes) // 4


def median_in_regs(nframes, NL):
    waves = SMED_WAVES_FEW if nframes <= SMED_FEW_FRAMES else SMED_WAVES_BATCH
    return NL <= 64 * waves * SMED_V


# ---- oracle side: one OracleExtractor per image (it keeps the image's pyramid), cached over the cases that share images ----
_ORA = {}


def oracle_of(img, ext):
    key = (hashlib.sha1(img.tobytes()).hexdigest(), img.shape, tuple(ext))
    if key not in _ORA:
        o = O.OracleExtractor(*ext)
        _, k, d = o(img)
        _ORA[key] = (o, k, d)
    return _ORA[key]


@functools.lru_cache(maxsize=None)
def level_table(size, ext):
    """(scale f32 [L], invScale f32 [L], [(w_l, h_l)]) of an extractor on an image of `size`."""
    o = O.OracleExtractor(*ext)
    o(np.zeros((size[1], size[0]), np.uint8))
    t = o.tables()
    return t["scale"], t["inv_scale"], [o.level_size(l) for l in range(ext[2])]


def oracle_matches(case, f):
    """(uRight, depth) of frame f by the oracle, float32 [NL]."""
    fr = case["frames"].get(f)
    if fr is None:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    ol, orr = oracle_of(fr["imgL"], case["ext"])[0], oracle_of(fr["imgR"], case["ext"])[0]
    return O.stereo_matches(ol, orr, fr["kl"], fr["dl"], fr["kr"], fr["dr"], case["mbf"], case["mb"])


def with_nframes(case, n):
    assert n > max(case["frames"])
    c = dict(case); c["nframes"] = n
    return c


def legal(case):
    """Every keypoint below its count is one the extractor could emit: 0 <= octave < nlevels and EDGE <= round(coordinate * invScale) <
    level size - EDGE on its own level.  A case that fails is a bug in the case, never something to try on the GPU."""
    scale, inv, sizes = level_table(case["size"], case["ext"])
    nl = case["ext"][2]
    assert case["cap"] < 65536 and case["nframes"] > max(case["frames"])
    for f, fr in case["frames"].items():
        assert fr["imgL"].shape == fr["imgR"].shape == (case["size"][1], case["size"][0]) and fr["imgL"].dtype == np.uint8
        for side in ("l", "r"):
            k, d = fr["k" + side], fr["d" + side]
            assert k.dtype == KP_DTYPE and d.dtype == np.uint8 and d.shape == (len(k), 32) and len(k) <= case["cap"], (case["name"], f, side)
            if not len(k):
                continue
            o = k["octave"]
            assert ((o >= 0) & (o < nl)).all(), (case["name"], f, side, "octave")
            w = np.array([sizes[i][0] for i in o]); h = np.array([sizes[i][1] for i in o])
            x = np.round(k["x"] * inv[o]); y = np.round(k["y"] * inv[o])   # float32 products, round half away from zero on .5 aside (positions are never at .5)
            bad = ~((x >= EDGE) & (x < w - EDGE) & (y >= EDGE) & (y < h - EDGE))
            assert not bad.any(), (case["name"], f, side, np.nonzero(bad)[0][:5], k[bad][:5])
    return True


# ---- the path mirror ----
def _right_rows(case, kr):
    scale = level_table(case["size"], case["ext"])[0]
    r = np.float32(2.0) * scale[kr["octave"]]
    return np.floor(kr["y"] - r).astype(np.int64), np.ceil(kr["y"] + r).astype(np.int64)


def _band_lists(case, f):
    """Per 16-row band the right keypoints k_stereo_prep registers in it (ascending index), and the list's total length."""
    fr = case["frames"][f]
    nRows = case["size"][1]
    nBands = (nRows + SM_BAND - 1) // SM_BAND
    minr, maxr = _right_rows(case, fr["kr"])
    lists = [[] for _ in range(nBands)]
    for iR in range(len(fr["kr"])):
        if maxr[iR] >= 0 and minr[iR] < nRows:
            for b in range(max(minr[iR], 0) // SM_BAND, min(maxr[iR], nRows - 1) // SM_BAND + 1):
                lists[b].append(iR)
    return [np.array(l, np.int64) for l in lists], sum(len(l) for l in lists)


def list_total(case, f):
    return _band_lists(case, f)[1] if f in case["frames"] else 0


def use_bands(case, f):
    nBands = (case["size"][1] + SM_BAND - 1) // SM_BAND
    return nBands <= SM_MAXB and list_total(case, f) <= SM_LIST * case["cap"]


def candidate_mask(case, f):
    """[NL, NR] bool: right keypoint iR passes left keypoint iL's gates (k_stereo_match stage A; the reference's vRowIndices[row] walk plus
    its octave and disparity tests): row in [floor(y - r), ceil(y + r)] with r = 2 scale[octR], |octR - octL| <= 1,
    uL - mbf / mb <= xR <= uL, and the row valid.  Float32 throughout, like the kernel."""
    fr = case["frames"][f]
    kl, kr = fr["kl"], fr["kr"]
    nRows = case["size"][1]
    minr, maxr = _right_rows(case, kr)
    maxD = np.float32(case["mbf"]) / np.float32(case["mb"])
    row = kl["y"].astype(np.int64)                       # (int)vL: the coordinates are positive
    minU = (kl["x"] - maxD).astype(np.float32)
    rowOk = (row >= 0) & (row < nRows) & ~(kl["x"] < 0)
    m = (row[:, None] >= minr[None]) & (row[:, None] <= maxr[None])
    m &= np.abs(kr["octave"][None].astype(np.int64) - kl["octave"][:, None]) <= 1
    m &= (kr["x"][None] >= minU[:, None]) & (kr["x"][None] <= kl["x"][:, None])
    return m & rowOk[:, None]


def pairs_per_scan(case, f, nframes=None):
    """Walks every wave of frame f the way stage A of k_stereo_match does at the workgroup shape of `nframes` (default: the case's) and returns
    dict(mid=number of mid-scan flushes, inside=those that cut a keypoint's run (pairs of one q on both sides), between=those after which the
    current keypoint adds nothing and a later keypoint of the wave does, maxPairs=most pairs a wave holds at a flush, maxCand=most candidates
    of one left keypoint, events=where the flushes of the two kinds fell)."""
    nframes = nframes or case["nframes"]
    out = dict(mid=0, inside=0, between=0, maxPairs=0, maxCand=0, events=[])   # events: (first left index of the workgroup, wave, q, kind)
    if f not in case["frames"]:
        return out
    fr = case["frames"][f]
    NL, NR = len(fr["kl"]), len(fr["kr"])
    lk = sm_lk_for(nframes); KQ = lk // 4
    cand = candidate_mask(case, f)
    banded = use_bands(case, f)
    lists = _band_lists(case, f)[0] if banded else None
    row = fr["kl"]["y"].astype(np.int64)
    nRows = case["size"][1]
    steps = []     # per left keypoint: pairs added by each 64-entry step of its scan
    for iL in range(NL):
        if not (0 <= row[iL] < nRows):
            steps.append(np.zeros(0, np.int64)); continue
        hits = cand[iL, lists[row[iL] // SM_BAND]] if banded else cand[iL]
        steps.append(np.add.reduceat(hits.astype(np.int64), np.arange(0, len(hits), 64)) if len(hits) else np.zeros(0, np.int64))
    out["maxCand"] = int(cand.sum(1).max()) if NL and NR else 0
    for iL0 in range(0, NL, lk):
        for wv in range(4):
            qs = [iL0 + q * 4 + wv for q in range(KQ) if iL0 + q * 4 + wv < NL]
            n = 0
            for a, iL in enumerate(qs):
                st = steps[iL]
                for s in range(len(st)):
                    n += int(st[s])
                    if n > SM_PCAP - 64:
                        out["mid"] += 1; out["maxPairs"] = max(out["maxPairs"], n)
                        before, after = int(st[:s + 1].sum()), int(st[s + 1:].sum())
                        if before and after:
                            out["inside"] += 1; out["events"].append((iL0, wv, a, "inside"))
                        elif not after and any(steps[j].sum() for j in qs[a + 1:]):
                            out["between"] += 1; out["events"].append((iL0, wv, a, "between"))
                        n = 0
            out["maxPairs"] = max(out["maxPairs"], n)
    assert out["maxPairs"] <= SM_PCAP
    return out


# ---- building blocks ----
def kp(x, y, octave, case_scale):
    k = np.zeros(1, KP_DTYPE)
    k["x"], k["y"], k["octave"] = np.float32(x), np.float32(y), octave
    k["size"], k["angle"], k["response"], k["class_id"] = np.float32(31.0) * case_scale[octave], 0.0, 1.0, -1
    return k


def thermo_low(d):
    """d bits set from the bottom: with thermo_high(e), distance e + d (e + d <= 256); two thermo_low codes are |d1 - d2| apart."""
    b = np.zeros(256, np.uint8); b[:d] = 1
    return np.packbits(b, bitorder="little")


def thermo_high(e):
    b = np.zeros(256, np.uint8); b[256 - e:] = 1 if e else 0
    return np.packbits(b, bitorder="little")


def _cat(parts, dtype, tail=()):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros((0,) + tuple(tail), dtype)


@functools.lru_cache(maxsize=None)
def base(size=(752, 480), ext=DEFAULT_EXT, seed=60, cam=None):
    """A synthetic stereo pair, what the (oracle) extractor finds in it, and its real stereo matches: the stock the cases rearrange."""
    from morb_slam_amd.synth import make_stereo_pair
    imgL, imgR = make_stereo_pair(size[0], size[1], seed=seed)
    (ol, kl, dl), (orr, kr, dr) = oracle_of(imgL, ext), oracle_of(imgR, ext)
    mbf, mb = cam or EUROC
    u, d = O.stereo_matches(ol, orr, kl, dl, kr, dr, mbf, mb)
    return dict(imgL=imgL, imgR=imgR, kl=kl, dl=dl, kr=kr, dr=dr, u=u, size=size, ext=ext, mbf=mbf, mb=mb)


def real_pairs(b, octaves=(0,), min_x=0.0, min_disp=6.0, max_disp=60.0):
    """Real matched left keypoints of the base pair with the right keypoint the oracle refined them from: [(iL, iR)] — the right keypoint of a
    compatible octave on the left's rows, closest to the refined uRight (the SAD search moves at most 5 level pixels)."""
    scale = level_table(b["size"], b["ext"])[0]
    c = dict(name="_", size=b["size"], ext=b["ext"], mbf=b["mbf"], mb=b["mb"], cap=65535, nframes=1,
             frames={0: dict(imgL=b["imgL"], imgR=b["imgR"], kl=b["kl"], dl=b["dl"], kr=b["kr"], dr=b["dr"])})
    cand = candidate_mask(c, 0)
    out = []
    for iL in np.nonzero(b["u"] >= 0)[0]:
        k = b["kl"][iL]
        if k["octave"] not in octaves or k["x"] < min_x or not (min_disp <= k["x"] - b["u"][iL] <= max_disp):
            continue
        js = np.nonzero(cand[iL])[0]
        if not len(js):
            continue
        j = js[np.argmin(np.abs(b["kr"]["x"][js] - b["u"][iL]))]
        if abs(b["kr"]["x"][j] - b["u"][iL]) <= 5.5 * scale[k["octave"]]:
            out.append((int(iL), int(j)))
    return out


def isolated_pairs(b, pairs, half, ymin=45.0):
    """A subset of `pairs` whose left rows are more than 2 * half apart (and clear of the first and last legal rows): with half chosen from
    the rows the gadgets' right keypoints register in, gadgets built on them cannot see each other.  The builders verify that with
    assert_isolated()."""
    taken, out = [], []
    for iL, iR in pairs:
        y = float(b["kl"]["y"][iL])
        if y < ymin or y > b["size"][1] - 1 - ymin:
            continue
        if all(abs(y - t) > 2 * half for t in taken):
            taken.append(y); out.append((iL, iR))
    return out


POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_rows(dl, dr):
    """[NL, NR] Hamming distances."""
    out = np.zeros((len(dl), len(dr)), np.int64)
    for i in range(len(dl)):
        out[i] = POPCOUNT[dl[i][None] ^ dr].sum(1)
    return out


def best_candidates(case, f):
    """Per left keypoint of frame f, from the inputs alone: (number of candidates, smallest candidate distance or 256, lowest right index at
    that distance or -1, how many candidates sit at that distance)."""
    fr = case["frames"][f]
    cand = candidate_mask(case, f)
    d = np.where(cand, hamming_rows(fr["dl"], fr["dr"]), 256)
    n = cand.sum(1)
    if d.shape[1] == 0:
        z = np.zeros(len(n), np.int64)
        return n, z + 256, z - 1, z
    best = d.min(1)
    idx = np.where(best < 256, d.argmin(1), -1)
    return n, best, idx, ((d == best[:, None]) & cand).sum(1)


def assert_isolated(case, f, owner):
    """owner[iR] = the left index right keypoint iR was built for: no left keypoint among the owners sees another's right keypoints."""
    cand = candidate_mask(case, f)
    owner = np.asarray(owner)
    for g in np.unique(owner):
        assert not cand[g, owner != g].any(), (case["name"], "gadget", int(g), "sees", np.nonzero(cand[g] & (owner != g))[0][:4])


def kp_legal(k, size, ext):
    scale, inv, sizes = level_table(size, ext)
    o = int(k["octave"][0])
    if not 0 <= o < ext[2]:
        return False
    x, y = np.round(k["x"][0] * inv[o]), np.round(k["y"][0] * inv[o])
    return bool(EDGE <= x < sizes[o][0] - EDGE and EDGE <= y < sizes[o][1] - EDGE)


def _case(name, b, frames, cap, nframes, classes=None, doc=""):
    return dict(name=name, size=b["size"], ext=b["ext"], mbf=b["mbf"], mb=b["mb"], cap=cap, nframes=nframes, frames=frames,
                classes=classes or {}, doc=doc)


def _frame(b, kl, dl, kr, dr, imgL=None, imgR=None):
    return dict(imgL=b["imgL"] if imgL is None else imgL, imgR=b["imgR"] if imgR is None else imgR,
                kl=np.ascontiguousarray(kl), dl=np.ascontiguousarray(dl), kr=np.ascontiguousarray(kr), dr=np.ascontiguousarray(dr))


# ---- the cases ----
@functools.lru_cache(maxsize=None)
def dense_rows():
    """One 752 x 480 frame with three heavy row bands, on top of the pair's real keypoints (which keep their real matches).  Each heavy group is
    eight left keypoints at the position of a real matched octave-0 keypoint (+ a column offset), so that the SAD refinement succeeds from the
    right keypoint that sits at the real partner's column and the result shows WHICH right keypoint won the Hamming stage:
      group A  left indices 4 q + 0 (wave 0 of workgroup 0 in the eight-per-wave shape); its band holds exactly 96 right keypoints and every one
               of them passes all gates of all eight: each scan adds 64 + 32 pairs whatever the band's order, the running count reaches
               448 after q = 4's first step (no flush: the test is >) and 480 after its second: a flush BETWEEN keypoints 4 and 5;
      group B  left indices 4 q + 1 (wave 1); 100 right keypoints: 64 + 36 per scan, 464 after q = 4's first step: a flush INSIDE q = 4's run;
      group C  left indices 4 q + 2 (wave 2); 640 right keypoints 0.7 px apart on one row, every one a candidate: with one keypoint per wave
               (one frame) the run of more than SM_PCAP pairs is cut by a flush in every order.
    Descriptors are thermometer codes: right j has d_j low bits, left i = its target's code with e_i high bits flipped, distance
    |d_t - d_j| + e_i.  Some d_j repeat the target's at a lower and at a higher right index (ties: the lower index must win, from either side
    of a flush).  The real right keypoints registered in bands A and B are dropped so that those bands hold only what is listed above."""
    b = base()
    scale = level_table(b["size"], b["ext"])[0]
    pairs = real_pairs(b, octaves=(0,), min_x=480.0, min_disp=12.0)
    # three real pairs in bands at least two apart, rows well inside their band (the right keypoints' five rows stay in one band)
    chosen = []
    for iL, iR in pairs:
        y = b["kl"]["y"][iL]
        if 3 <= int(y) % SM_BAND <= 12 and all(abs(int(y) // SM_BAND - int(b["kl"]["y"][c[0]]) // SM_BAND) >= 2 for c in chosen):
            chosen.append((iL, iR))
        if len(chosen) == 3:
            break
    assert len(chosen) == 3, "the base pair has no three separate real matches to build on"
    minr, maxr = _right_rows(dict(size=b["size"], ext=b["ext"]), b["kr"])
    drop = np.zeros(len(b["kr"]), bool)
    for iL, _ in chosen[:2]:
        bnd = int(b["kl"]["y"][iL]) // SM_BAND
        drop |= (np.maximum(minr, 0) // SM_BAND <= bnd) & (np.minimum(maxr, b["size"][1] - 1) // SM_BAND >= bnd)
    krReal, drReal = b["kr"][~drop], b["dr"][~drop]
    rng = np.random.default_rng(11)
    heavyL = {}                       # left index -> (keypoint, descriptor)
    krs, drs = [krReal], [drReal]
    nR = len(krReal)
    classes = {"A": [], "B": [], "C": []}
    offs = [-2, -1, 0, 1, 2, 0, 1, -1]
    es = [0, 3, 10, 24, 1, 40, 7, 60]
    for g, (wv, nright, step) in enumerate(((0, 96, 3.0), (1, 100, 3.0), (2, 640, 0.7))):
        iL, iR = chosen[g]
        x0, y0, xp = float(b["kl"]["x"][iL]), float(b["kl"]["y"][iL]), float(b["kr"]["x"][iR])
        # right keypoints of the group: five targets at the partner's column + offset, then fillers going left; all <= the smallest uL
        # and >= the largest uL - mbf / mb
        xs = [xp + o for o in (-2, -1, 0, 1, 2)]
        xs += [x0 - 2 - 64 - step * k for k in range(nright - 5)] if g < 2 else [x0 - 2.35 - step * k for k in range(nright - 5)]
        ds = [10, 20, 30, 40, 50] + [int(v) for v in rng.integers(118, 190, nright - 5)]
        # ties: repeat the first three targets' codes in two fillers each; shuffle the group so that targets and their ties take any relative index order
        for t in range(3):
            ds[5 + 2 * t] = ds[t]; ds[6 + 2 * t] = ds[t]
        perm = rng.permutation(nright)
        xs, ds = [xs[p] for p in perm], [ds[p] for p in perm]
        tgt = {t: int(np.nonzero(perm == t)[0][0]) for t in range(5)}
        for x, d in zip(xs, ds):
            krs.append(kp(x, y0, 0, scale)); drs.append(thermo_low(d)[None])
        for q in range(8):
            t = offs[q] + 2
            heavyL[4 * q + wv] = (kp(x0 + offs[q], y0, 0, scale), (thermo_low(ds[tgt[t]]) ^ thermo_high(es[q]))[None])
            classes["ABC"[g]].append((0, 4 * q + wv))
        nR += nright
    # left side: heavy keypoints at their indices, the real ones everywhere else
    NL = len(b["kl"]) + len(heavyL)
    kl = np.zeros(NL, KP_DTYPE); dl = np.zeros((NL, 32), np.uint8)
    it = iter(range(len(b["kl"])))
    for i in range(NL):
        if i in heavyL:
            kl[i], dl[i] = heavyL[i][0][0], heavyL[i][1][0]
        else:
            j = next(it); kl[i], dl[i] = b["kl"][j], b["dl"][j]
    fr = _frame(b, kl, dl, _cat(krs, KP_DTYPE), _cat(drs, np.uint8, (32,)))
    return _case("dense_rows", b, {0: fr}, cap=2100, nframes=1, classes=classes, doc=dense_rows.__doc__)


def dense_row_1():
    c = dict(dense_rows()); c["name"] = "dense_row_1"; c["nframes"] = 1
    return c


def dense_row_8():
    c = dict(dense_rows()); c["name"] = "dense_row_8"; c["nframes"] = 33
    return c


_LEVELS = {}


def _level(img, ext, lvl):
    key = (id(img), tuple(ext), lvl)
    if key not in _LEVELS:
        _LEVELS[key] = oracle_of(img, ext)[0].level_image(lvl).astype(np.int64)     # the level with its 19-pixel border
    return _LEVELS[key]


def sad_distance(case, f, iL, iR):
    """The SAD stage's best distance for left keypoint iL refined from right keypoint iR (the smallest of the 11 shifts' 11 x 11 L1 norms on the
    un-blurred level of the left octave), or None when the strip leaves the level: what k_stereo_median sorts."""
    fr = case["frames"][f]
    scale, inv, sizes = level_table(case["size"], case["ext"])
    o = int(fr["kl"]["octave"][iL])
    rnd = lambda v: int(np.floor(np.float32(v) * inv[o] + np.float32(0.5)))
    u, v, uR = rnd(fr["kl"]["x"][iL]), rnd(fr["kl"]["y"][iL]), rnd(fr["kr"]["x"][iR])
    if uR < 0 or uR + 11 >= sizes[o][0]:
        return None
    IL, IR = _level(fr["imgL"], case["ext"], o), _level(fr["imgR"], case["ext"], o)
    P = IL[EDGE + v - 5:EDGE + v + 6, EDGE + u - 5:EDGE + u + 6]
    return min(int(np.abs(P - IR[EDGE + v - 5:EDGE + v + 6, EDGE + uR + inc - 5:EDGE + uR + inc + 6]).sum()) for inc in range(-5, 6))


def median_cut(dists):
    """The cut of Frame.cc:1036-1047 on the accepted SAD distances: (median, [cut?]) — sorted[size / 2], threshold 1.5f * 1.4f * median."""
    d = np.asarray(dists)
    median = int(np.sort(d)[len(d) // 2])
    th = np.float32(1.5) * np.float32(1.4) * np.float32(median)
    return median, ~(d.astype(np.float32) < th)


@functools.lru_cache(maxsize=None)
def _median_stock():
    """Per left keypoint of the base pair: accepted by the SAD stage when matched alone (a lone match is its own median and is never cut), and
    its SAD distance."""
    b = base()
    c = _case("_", b, {0: _frame(b, b["kl"], b["dl"], b["kr"], b["dr"])}, cap=65535, nframes=1)
    ol, orr = oracle_of(b["imgL"], b["ext"])[0], oracle_of(b["imgR"], b["ext"])[0]
    _, best, idx, _ = best_candidates(c, 0)
    acc = np.zeros(len(b["kl"]), bool); dist = np.full(len(b["kl"]), -1, np.int64)
    for i in np.nonzero(best < (TH_HIGH + TH_LOW) // 2)[0]:
        acc[i] = O.stereo_matches(ol, orr, b["kl"][i:i + 1], b["dl"][i:i + 1], b["kr"], b["dr"], b["mbf"], b["mb"])[0][0] >= 0
        if acc[i]:
            dist[i] = sad_distance(c, 0, i, idx[i])
    return acc, dist


@functools.lru_cache(maxsize=None)
def median_global():
    """17 frames (k_stereo_median<4>: 2048 distances in registers), frame 0 with 2100 left keypoints, so the median runs on its global-memory
    form.  The left side is the base pair's keypoints plus copies, arranged so that the path is worth running:
      * copies of the keypoint with the smallest SAD distance pull the median down to a value m for which an accepted distance lies in
        [2.1 m, 2.1 (m + 1)): a median off by one changes which keypoints are cut (case["median"] holds m, the distances and the cut);
      * the base keypoints come LAST, rotated so that keypoints which the median cuts sit at indices beyond 2048: a pass that stops at what
        the registers would hold leaves them uncut;
      * the rest are copies of keypoints that match nothing."""
    b = base()
    acc, dist = _median_stock()
    n = len(b["kl"])
    D = np.sort(dist[acc]); T = len(D)
    lo = int(np.nonzero(acc)[0][np.argmin(dist[acc])])
    extra = 2100 - n
    pick = None
    for t in range(T // 2, max((T - extra) // 2, 0), -1):        # adding c copies of the smallest moves the median to D[(T + c) / 2 - c]
        c = T - 2 * t
        if not (0 <= c <= extra and (T + c) // 2 - c == t):
            continue
        m = int(D[t]); th, th1 = np.float32(1.5) * np.float32(1.4) * np.float32(m), np.float32(1.5) * np.float32(1.4) * np.float32(m + 1)
        if ((D.astype(np.float32) >= th) & (D.astype(np.float32) < th1)).any():
            pick = (c, m); break
    assert pick, "no reachable median has an accepted distance in its off-by-one window"
    c, m = pick
    none = np.nonzero(~acc)[0]
    cutBase = acc & ~(dist.astype(np.float32) < np.float32(1.5) * np.float32(1.4) * np.float32(m))
    last = int(np.nonzero(cutBase)[0][-1])
    rot = np.roll(np.arange(n), n - 1 - last - 5)                 # the last cut keypoint ends five from the end
    idx = np.concatenate([np.full(c, lo), none[np.arange(extra - c) % len(none)], rot])
    fr = _frame(b, b["kl"][idx], b["dl"][idx], b["kr"], b["dr"])
    case = _case("median_global", b, {0: fr}, cap=2304, nframes=17, doc=median_global.__doc__)
    case["median"] = dict(m=m, acc=acc[idx], dist=dist[idx])
    return case


HD = ((1920, 1080), (400, 1.9, 5, 20, 7), (np.float32(1400.0 * 0.12), np.float32(0.12)))


@functools.lru_cache(maxsize=None)
def _hd_sets():
    """1920 x 1080, scale factor 1.9, 5 levels, capacity 512 = the right count.  (Scale factor 2.0 would do on the oracle, but its level 4 is
    120 x 68 and the extractor builds no level under 76 px; at 1.9 level 4 is 147 x 83.)  An octave-4 keypoint registers in 2 * 26 + 1 rows
    and more: four or five 16-row bands, so 512 right keypoints mostly of octave 4 pass SM_LIST * cap list entries.  Right side: the
    partners of the pair's real matches (so the frame keeps real matches), then constructed octave-4 keypoints at integer level coordinates
    — on level rows that cover five bands — with random descriptors.
    Returns the base and three right sets: unbanded (every filler of octave 4), and two states of one set trimmed to listTotal == 4 cap
    and 4 cap + 1: fillers swapped for octave-0 keypoints in the middle of a band (one band each) until the total is at or under 4 cap,
    some of those moved to the band's last row (two bands, + 1 each) to land on 4 cap, and one more moved between the two states."""
    size, ext, cam = HD
    b = base(size, ext, 61, cam)
    scale, inv, sizes = level_table(size, ext)
    cap = 512
    pairs = real_pairs(b, octaves=(0, 1, 2, 3, 4), min_disp=2.0, max_disp=160.0)
    keepR = sorted({iR for _, iR in pairs})[:120]

    def total(k):
        return list_total(dict(size=size, ext=ext, cap=cap, frames={0: dict(kr=k)}), 0)
    rng = np.random.default_rng(5)
    w4, h4 = sizes[4]
    rows5 = [ky for ky in range(EDGE, h4 - EDGE) if total(kp(400.0, np.float32(ky) * scale[4], 4, scale)) == 5]
    assert len(rows5) >= 8
    nfill = cap - len(keepR)
    fx = rng.integers(EDGE, w4 - EDGE, nfill).astype(np.float32) * scale[4]
    fy = rng.choice(rows5, nfill).astype(np.float32) * scale[4]
    fill = _cat([kp(x, y, 4, scale) for x, y in zip(fx, fy)], KP_DTYPE)
    fdesc = rng.integers(0, 256, (nfill, 32), dtype=np.uint8)
    kr = _cat([b["kr"][keepR], fill], KP_DTYPE); dr = _cat([b["dr"][keepR], fdesc], np.uint8, (32,))
    T = total(kr)
    assert T > SM_LIST * cap + 12, T
    edge = kr.copy()
    j = len(keepR)
    one = lambda i, r: kp(float(edge["x"][i]), float(16 * int(edge["y"][i] // 16) + r), 0, scale)[0]   # row 16 m + 8: one band; 16 m + 15: two
    n1 = 0
    while total(edge) > SM_LIST * cap:
        edge[j + n1] = one(j + n1, 8); n1 += 1
    deficit = SM_LIST * cap - total(edge)
    assert 0 <= deficit < n1 - 1
    for i in range(deficit):
        edge[j + 1 + i] = one(j + 1 + i, 15)
    assert total(edge) == SM_LIST * cap
    over = edge.copy()
    over[j] = one(j, 15)                                         # across the band border: + 1
    assert total(over) == SM_LIST * cap + 1
    return b, cap, dr, kr, edge, over, j


def unbanded():
    b, cap, dr, kr, _, _, _ = _hd_sets()
    return _case("unbanded", b, {0: _frame(b, b["kl"], b["dl"], kr, dr)}, cap=cap, nframes=1, doc=_hd_sets.__doc__)


def banded_edge():
    """Two frames of one batch: the same keypoint set with listTotal == 4 cap (frame 0: bands used) and 4 cap + 1 (frame 1: not used); see _hd_sets."""
    b, cap, dr, _, edge, over, j = _hd_sets()
    return _case("banded_edge", b, {0: _frame(b, b["kl"], b["dl"], edge, dr), 1: _frame(b, b["kl"], b["dl"], over, dr)}, cap=cap, nframes=2,
                 classes={"moved": [(0, j), (1, j)]}, doc=banded_edge.__doc__)


def _gadget_frame(b, gadgets, extraL=()):
    """gadgets: [(left keypoint, left descriptor, [(right keypoint, right descriptor), ...])] -> frame with only these keypoints; the left index
    of gadget g is g (extraL follow)."""
    kl = _cat([g[0] for g in gadgets] + [e[0] for e in extraL], KP_DTYPE)
    dl = _cat([g[1][None] for g in gadgets] + [e[1][None] for e in extraL], np.uint8, (32,))
    kr = _cat([r[0] for g in gadgets for r in g[2]], KP_DTYPE)
    dr = _cat([r[1][None] for g in gadgets for r in g[2]], np.uint8, (32,))
    return kl, dl, kr, dr


@functools.lru_cache(maxsize=None)
def thresholds():
    """The Hamming gates at equality, one gadget per real matched pair (left keypoint at the real left position, right keypoints at the real
    partner's column unless stated), gadgets on disjoint rows so that each sees only its own right keypoints.  Left descriptors are all zero,
    a right descriptor thermo_low(d) is d away.  Classes (the class list holds the gadgets' left indices):
      best74       one candidate at 74: passes the (TH_HIGH + TH_LOW) / 2 gate           best75   one at 75: fails it
      best99       candidates at 99 and 120: 99 becomes the best, fails the 75 gate      only100  one at 100: never a best
      tie_low_at_partner   two at distance 20, the lower index at the partner's column, the higher 24 px left of it
      tie_low_elsewhere    the same, the lower index 24 px left
      tie_many     130 candidates 0.5 px apart, three of them at the minimum: more than one 64-pair round in every workgroup shape
    The tie "with the lower index arriving in a later round / flush" cannot be aimed at: inside a band the list order is the arrival order of
    k_stereo_prep's atomics.  tie_many (rounds) and dense_rows (flushes) put ties where both orders occur."""
    b = base()
    scale = level_table(b["size"], b["ext"])[0]
    iso = isolated_pairs(b, real_pairs(b, octaves=(0, 1), min_x=170.0, min_disp=8.0), half=float(scale[2]) + 1.0)
    kinds = ["best74", "best75", "best99", "only100", "tie_low_at_partner", "tie_low_elsewhere", "tie_many"]
    assert len(iso) >= 4 * len(kinds), len(iso)
    z = np.zeros(32, np.uint8)
    gadgets, classes = [], {k: [] for k in kinds}
    for g, (iL, iR) in enumerate(iso[:5 * len(kinds)]):
        kind = kinds[g % len(kinds)]
        kL, kR = b["kl"][iL:iL + 1], b["kr"][iR:iR + 1]
        o = int(kR["octave"][0]); xp, y = float(kR["x"][0]), float(kR["y"][0])
        at = lambda x: kp(x, y, o, scale)
        if kind == "best74": rs = [(at(xp), thermo_low(74))]
        elif kind == "best75": rs = [(at(xp), thermo_low(75))]
        elif kind == "best99": rs = [(at(xp - 24), thermo_low(120)), (at(xp), thermo_low(99))]
        elif kind == "only100": rs = [(at(xp), thermo_low(100))]
        elif kind == "tie_low_at_partner": rs = [(at(xp), thermo_low(20)), (at(xp - 24), thermo_low(20))]
        elif kind == "tie_low_elsewhere": rs = [(at(xp - 24), thermo_low(20)), (at(xp), thermo_low(20))]
        else:
            rs = [(at(xp - 0.5 * k), thermo_low(90 - (k % 50))) for k in range(1, 128)]     # 41 .. 90; the minimum 41 three times below
            rs.insert(100, (at(xp - 70.0), thermo_low(30))); rs.insert(40, (at(xp), thermo_low(30))); rs.insert(70, (at(xp - 71.0), thermo_low(30)))
        gadgets.append((kL, z, rs)); classes[kind].append((0, g))
    kl, dl, kr, dr = _gadget_frame(b, gadgets)
    c = _case("thresholds", b, {0: _frame(b, kl, dl, kr, dr)}, cap=1000, nframes=1, classes=classes, doc=thresholds.__doc__)
    assert_isolated(c, 0, [g for g, gd in enumerate(gadgets) for _ in gd[2]])
    return c


def _f32_next(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def geometry_gates():
    """The candidate gates at equality; gadgets as in thresholds(), one right keypoint each with the left's descriptor (distance 0), so a gadget
    whose right keypoint passes the gates goes on to the SAD stage and one whose does not stays unmatched.  Classes, `_in` passes, `_out` fails:
      minr_in / minr_out   the left row equals the right keypoint's floor(y - r) / lies one row above it
      maxr_in / maxr_out   the left row equals ceil(y + r) / lies one row below it
      oct_m1 oct_p1 (in), oct_m2 oct_p2 (out)   right octave = left octave - 1, + 1, - 2, + 2 (left octaves 2 .. 5)
      xr_eq_ul (in), xr_above_ul (out)          xR == uL, xR one float step above uL
      xmin_eq xmin_above (in), xmin_below (out) xR at float32(uL - mbf / mb), one step above, one step below
      row19 / row_hm20     constructed left keypoints on the first and last legal rows (19 and h - 20), their right keypoint where the SAD search accepts it"""
    b = base()
    scale, inv, sizes = level_table(b["size"], b["ext"])
    maxD = np.float32(b["mbf"]) / np.float32(b["mb"])
    # a right keypoint of octave <= 7 moved r + 1.25 rows off the left row registers up to 2 r + 2.25 + 1 rows from it
    # (the scarce pairs of octaves 2 .. 5 first, so that the isolation does not crowd them out)
    pairs = real_pairs(b, octaves=(0, 1, 2, 3, 4, 5), min_x=150.0, min_disp=8.0)
    pairs = [p for p in pairs if b["kl"]["octave"][p[0]] >= 2][:10] + [p for p in pairs if b["kl"]["octave"][p[0]] < 2]
    pool = isolated_pairs(b, pairs, half=float(scale[7]) + 2.0)
    kinds = ["oct_m1", "oct_p1", "oct_m2", "oct_p2", "xmin_eq", "xmin_above", "xmin_below", "minr_in", "minr_out", "maxr_in", "maxr_out",
             "xr_eq_ul", "xr_above_ul"]
    gadgets, classes = [], {k: [] for k in kinds + ["row19", "row_hm20"]}
    used = set()
    for kind in kinds * 2 + ["minr_in", "maxr_in"] * 2:     # (a few more of the kinds that end in a match)
        for n, (iL, iR) in enumerate(pool):
            if n in used:
                continue
            kL = b["kl"][iL:iL + 1]; dL = b["dl"][iL]
            oL, oR = int(kL["octave"][0]), int(b["kr"]["octave"][iR])
            uL = np.float32(kL["x"][0]); row = int(kL["y"][0])
            x, y, o = float(b["kr"]["x"][iR]), float(kL["y"][0]), oR
            r = float(np.float32(2.0) * scale[oR])
            if kind.startswith("oct"):
                if not 2 <= oL <= 5:
                    continue
                o = oL + {"oct_m1": -1, "oct_p1": 1, "oct_m2": -2, "oct_p2": 2}[kind]
            elif oL > 1:
                continue
            elif kind.startswith("minr"):
                y = np.float32(row + r + 0.25 + (1.0 if kind == "minr_out" else 0.0))     # floor(y - r) = row (+ 1)
            elif kind.startswith("maxr"):
                y = np.float32(row - r - 0.25 - (1.0 if kind == "maxr_out" else 0.0))     # ceil(y + r) = row (- 1)
            elif kind == "xr_eq_ul": x = uL
            elif kind == "xr_above_ul": x = _f32_next(uL, True)
            elif kind == "xmin_eq": x = np.float32(uL - maxD)
            elif kind == "xmin_above": x = _f32_next(np.float32(uL - maxD), True)
            elif kind == "xmin_below": x = _f32_next(np.float32(uL - maxD), False)
            kR = kp(x, y, o, scale)
            if not kp_legal(kR, b["size"], b["ext"]):
                continue
            used.add(n)
            gadgets.append((kL, dL, [(kR, dL)])); classes[kind].append((0, len(gadgets) - 1))
            break
    # first and last legal rows: constructed octave-0 keypoints (isolated_pairs keeps the gadgets 45 rows clear of them)
    extra = []
    for kind, y in (("row19", 19.0), ("row_hm20", float(b["size"][1] - 20))):
        d = thermo_low(3)
        # a column and a disparity at which the pair's images really agree on that row: the first the oracle accepts
        for x, dx in ((float(x), dx) for x in range(200, 700, 37) for dx in range(2, 61)):
            g = (kp(x, y, 0, scale), d, [(kp(x - dx, y, 0, scale), d)])
            if oracle_matches(_case("_", b, {0: _frame(b, *_gadget_frame(b, [g]))}, cap=1, nframes=1), 0)[0][0] >= 0:
                break
        extra.append(g)
        classes[kind].append((0, len(gadgets) + len(extra) - 1))
    gadgets += extra
    kl, dl, kr, dr = _gadget_frame(b, gadgets)
    c = _case("geometry_gates", b, {0: _frame(b, kl, dl, kr, dr)}, cap=160, nframes=1, classes=classes, doc=geometry_gates.__doc__)
    assert_isolated(c, 0, [g for g, gd in enumerate(gadgets) for _ in gd[2]])
    return c


PASSING_GATES = ("minr_in", "maxr_in", "oct_m1", "oct_p1", "xr_eq_ul", "xmin_eq", "xmin_above", "row19", "row_hm20")
FAILING_GATES = ("minr_out", "maxr_out", "oct_m2", "oct_p2", "xr_above_ul", "xmin_below")


@functools.lru_cache(maxsize=None)
def few_matches():
    """Five frames that end with 0 (keypoints, none accepted: the median's total == 0 return), 1, 2, 3 and 4 accepted matches before the median
    cut, every accepted match the SAME gadget repeated (a real matched pair: equal SAD distances, so the median is that distance for every
    k = total / 2 and nothing is cut), and a sixth with 3 copies of one pair and 1 of another pair."""
    b = base()
    iso = isolated_pairs(b, real_pairs(b, octaves=(0, 1), min_disp=8.0), half=4.0)
    (iL, iR), (jL, jR) = iso[0], iso[1]
    good = (b["kl"][iL:iL + 1], b["dl"][iL], [(b["kr"][iR:iR + 1], b["dl"][iL])])
    good2 = (b["kl"][jL:jL + 1], b["dl"][jL], [(b["kr"][jR:jR + 1], b["dl"][jL])])
    bad = (b["kl"][iL:iL + 1], np.zeros(32, np.uint8), [(b["kr"][iR:iR + 1], thermo_low(75))])
    frames, classes = {}, {}
    for f, gs in enumerate(([bad] * 3, [good], [good] * 2, [good] * 3, [good] * 4, [good] * 3 + [good2])):
        kl, dl, kr, dr = _gadget_frame(b, gs)
        frames[f] = _frame(b, kl, dl, kr[:1] if f < 5 else kr[[0, 3]], dr[:1] if f < 5 else dr[[0, 3]])
        classes["accepted_%d" % f if f < 5 else "accepted_3_and_1"] = [(f, i) for i in range(len(gs))]
    return _case("few_matches", b, frames, cap=70, nframes=6, classes=classes, doc=few_matches.__doc__)


@functools.lru_cache(maxsize=None)
def sad_edges():
    """The SAD and parabola gates on hand-made patches painted into BOTH images of the base pair (octave-0 keypoints only; the pair's real
    keypoints outside the painted block keep their real matches).  Right descriptor = left descriptor, so every gadget reaches the SAD stage.
      stripes, period 2, left == right:
        equal_sad_first  right keypoint an even number of columns left of uL: the SAD is 0 at shifts -4, -2, 0, 2, 4; the first must win
                         (bestincR = -4, accepted with SAD distance 0)
        inc_m5           an odd number of columns: zeros at -5, -3, ..: bestincR = -5, rejected
      V-shaped ramp |x - c| * 6, left == right:
        inc_p5           left at c, right keypoint at c - 5: the only zero is at shift +5, rejected
        disp_zero        left and right keypoint at c: unique minimum at shift 0 with dist1 == dist3, deltaR = 0, disparity exactly 0:
                         the 0.01 branch
      V-shaped ramp, the right image's ramp 3 columns further right:
        disp_negative    left and right keypoint at c: best shift +3, bestuR > uL, rejected by disparity >= 0
    Unreachable with any input, hence no class: dist1 + dist3 == 2 dist2 (NaN / infinite deltaR) and |deltaR| near 1.  The best shift is the
    FIRST smallest, so dist1 > dist2 strictly and dist3 >= dist2: with a = dist1 - dist2 > 0, b = dist3 - dist2 >= 0 the parabola gives
    deltaR = (a - b) / (2 (a + b)), which is finite and lies in (-0.5, 0.5].  The `deltaR < -1 || deltaR > 1` test never fires."""
    b = base()
    scale = level_table(b["size"], b["ext"])[0]
    imgL, imgR = b["imgL"].copy(), b["imgR"].copy()
    X0, X1, Y0 = 80, 400, 60            # three blocks of 40 rows, columns X0 .. X1
    xs = np.arange(X0, X1)
    cV = 250
    stripes = np.where(xs % 2 == 0, 0, 255).astype(np.uint8)
    vee = np.clip(np.abs(xs - cV) * 6, 0, 255).astype(np.uint8)
    veeR = np.clip(np.abs(xs - (cV + 3)) * 6, 0, 255).astype(np.uint8)
    imgL[Y0:Y0 + 40, X0:X1] = stripes; imgR[Y0:Y0 + 40, X0:X1] = stripes
    imgL[Y0 + 40:Y0 + 80, X0:X1] = vee; imgR[Y0 + 40:Y0 + 80, X0:X1] = vee
    imgL[Y0 + 80:Y0 + 120, X0:X1] = vee; imgR[Y0 + 80:Y0 + 120, X0:X1] = veeR
    yS, yV, yW = Y0 + 20.0, Y0 + 60.0, Y0 + 100.0
    specs = [("equal_sad_first", 300.0, yS - 8, 300.0 - 40), ("equal_sad_first", 301.0, yS + 8, 301.0 - 22), ("inc_m5", 300.0, yS, 300.0 - 41),
             ("inc_p5", float(cV), yV - 8, cV - 5.0), ("disp_zero", float(cV), yV + 8, float(cV)), ("disp_negative", float(cV), yW, float(cV))]
    # the real keypoints away from the painted block (their patches and descriptors are what the unpainted images gave: the oracle extractor
    # of the painted images is only asked for its pyramid)
    far = lambda k: ~((k["x"] > X0 - 40) & (k["x"] < X1 + 40) & (k["y"] > Y0 - 40) & (k["y"] < Y0 + 160))
    mL, mR = far(b["kl"]), far(b["kr"])
    gadgets, classes = [], {}
    for n, (kind, x, y, xr) in enumerate(specs):
        d = thermo_low(5 + n)
        gadgets.append((kp(x, y, 0, scale), d, [(kp(xr, y, 0, scale), d)])); classes.setdefault(kind, []).append((0, n))
    kl, dl, kr, dr = _gadget_frame(b, gadgets)
    fr = _frame(b, _cat([kl, b["kl"][mL]], KP_DTYPE), _cat([dl, b["dl"][mL]], np.uint8, (32,)), _cat([kr, b["kr"][mR]], KP_DTYPE),
                _cat([dr, b["dr"][mR]], np.uint8, (32,)), imgL, imgR)
    return _case("sad_edges", b, {0: fr}, cap=1300, nframes=1, classes=classes, doc=sad_edges.__doc__)


CASES = dict(dense_row_1=dense_row_1, dense_row_8=dense_row_8, median_global=median_global, unbanded=unbanded, banded_edge=banded_edge,
             thresholds=thresholds, sad_edges=sad_edges, few_matches=few_matches, geometry_gates=geometry_gates)
EVERY_SHAPE = ("dense_row_1", "dense_row_8", "thresholds")   # run at every frame count of WORKGROUP_SHAPES
