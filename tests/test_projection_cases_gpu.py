"""The constructed threshold cases of projection_cases.py through the Python entry points of morb_slam_amd/matcher.py, against the CPU oracle: tables,
counts, levels and flags equal, the frustum's floats equal by bits (or both NaN).  The entries with a k_search form (last, kf, mps, fuse, fuse_sim3,
sim3dir) run every problem on all three implementations with the same small frames — tier 1 at the natural capacity 128, tier 2 padded into capacity
2032 tensors, tier 3 with MORB_SERIAL_RESOLVE set — after asserting the tier through tests/search_tiers.py; the three must give identical tables.
Every batch mixes the case frames with an empty frame and a one-feature frame, and the in/out tables keep a sentinel past each frame's count."""
import numpy as np
import pytest

import projection_cases as PC
import search_tiers as T

pytestmark = pytest.mark.gpu

SENT = -7777
TIERS = (("tier1", 128, 1, False), ("tier2", 2032, 2, False), ("tier3", 128, 3, True))


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad(a, n, fill=0):
    a = np.asarray(a)
    assert len(a) <= n
    return np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])


def _stack(rows, n, fill=0):
    return _cu(np.stack([_pad(r, n, fill) for r in rows]))


def _pool(frames, cap):
    """frames: [(KP records, descriptors)] -> device kps [nimg, cap, 28], desc [nimg, cap, 32], count [nimg]."""
    kps = np.zeros((len(frames), cap, 28), np.uint8); desc = np.zeros((len(frames), cap, 32), np.uint8)
    for i, (k, d) in enumerate(frames):
        kps[i, :len(k)] = np.ascontiguousarray(k).view(np.uint8).reshape(-1, 28); desc[i, :len(k)] = d
    return _cu(kps), _cu(desc), _cu(np.array([len(k) for k, _ in frames], np.int32))


def _cut(p, n, keys=("k", "d", "ur", "flag", "init")):
    """Problem p searched in the first n features of its frame (the empty and the one-feature frame); no hand-written expectation: the oracle's."""
    q = dict(p)
    for key in keys:
        q[key] = p[key][:n]
    q["name"] = "%s_first%d" % (p["name"], n)
    q["expect"] = None
    return q


def _groups(problems, keys):
    out = {}
    for p in problems:
        out.setdefault(tuple(p[k] for k in keys), []).append(p)
    return out.values()


def _with_edges(ps):
    return list(ps) + [_cut(ps[0], 0), _cut(ps[0], 1)]


def _tier(entry, cap, want, serial, monkeypatch, mpCap=None):
    assert T.entry_tier(entry, cap, mpCap, serial) == want, (entry, cap, mpCap, serial)
    if serial:
        monkeypatch.setenv("MORB_SERIAL_RESOLVE", "1")
    else:
        monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)


def _table(got, n, p, o, init=None):
    """One problem's table: equal to the oracle's below the count, the sentinel above it, and (where written) the hand-written expectation."""
    np.testing.assert_array_equal(got[:n], o["table"], err_msg=p["name"])
    if init is not None:
        np.testing.assert_array_equal(got[n:], init[n:], err_msg=p["name"] + ": rows past the count")
    if p.get("expect") is not None:
        np.testing.assert_array_equal(got[:n], p["expect"], err_msg=p["name"] + " (hand-written)")


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), what


def _all_tiers(entry, run, groups, monkeypatch, q_is_mp=False):
    import torch
    for ps in groups:
        first = None
        for name, cap, want, serial in TIERS:
            _tier(entry, cap, want, serial, monkeypatch, cap if q_is_mp else None)
            try:
                out = run(ps, cap)
                torch.cuda.synchronize()
            finally:
                monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)
            if first is None:
                first = out
            else:
                _same(first, out, (entry, ps[0]["name"], name))


# ---- Frame::isInFrustum ----------------------------------------------------------------------------------------------------------------------
def _float_bits_equal(g, e, what):
    g, e = np.asarray(g, np.float32), np.asarray(e, np.float32)
    both_nan = np.isnan(g) & np.isnan(e)
    same = g.view(np.uint32) == e.view(np.uint32)
    assert (both_nan | same).all(), (what, g[~(both_nan | same)], e[~(both_nan | same)])


def _run_frustum(m, ps, mpCap=300, nrows=290):
    """The problems of one pyramid as frames of one call; each problem's rows are repeated to nrows > 256, so the second block of k_frustum works too."""
    import torch
    tiled = []
    for p in ps:
        idx = np.arange(nrows) % len(p["Pw"])
        tiled.append(dict(p, Pw=p["Pw"][idx], normal=p["normal"][idx], maxD=p["maxD"][idx], minD=p["minD"][idx], idx=idx))
    F = len(tiled)
    out = dict(inView=torch.full((F, mpCap), 7, dtype=torch.uint8, device="cuda"), level=torch.full((F, mpCap), SENT, dtype=torch.int32, device="cuda"))
    for k in ("projX", "projY", "projXR", "depth", "viewCos"):
        out[k] = torch.full((F, mpCap), float(SENT), device="cuda")
    P = PC.params(ps[0]["pyr"])
    trk = m.isInFrustum(P, _cu(np.stack([p["R"] for p in tiled])), _cu(np.stack([p["t"] for p in tiled])), _cu(np.stack([p["Ow"] for p in tiled])),
                        _cu(np.full(F, nrows, np.int32)), _stack([p["Pw"] for p in tiled], mpCap), _stack([p["normal"] for p in tiled], mpCap),
                        _stack([p["maxD"] for p in tiled], mpCap, 1), _stack([p["minD"] for p in tiled], mpCap, 1), ps[0]["cosLimit"], out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in trk.items()}
    for f, p in enumerate(tiled):
        e = PC.oracle(p)["trk"]
        for k in ("inView", "level"):
            np.testing.assert_array_equal(got[k][f, :nrows], e[k], err_msg=p["name"] + " " + k)
            assert (got[k][f, nrows:] == (7 if k == "inView" else SENT)).all(), (p["name"], k, "rows past the count")
        for k in ("projX", "projY", "projXR", "depth", "viewCos"):
            _float_bits_equal(got[k][f, :nrows], e[k], (p["name"], k))
            assert (got[k][f, nrows:] == float(SENT)).all(), (p["name"], k, "rows past the count")
        n0 = len(ps[f]["Pw"])
        np.testing.assert_array_equal(got["inView"][f, :n0], ps[f]["expect"], err_msg=p["name"] + " (hand-written)")
        for i, lv in ps[f]["level"].items():
            assert got["level"][f, i] == lv, (p["name"], i)
        for i in ps[f]["nan_rows"]:
            assert np.isnan(got["projX"][f, i]) and np.isnan(got["projY"][f, i])


def test_frustum_thresholds():
    from morb_slam_amd import ORBmatcher
    m = ORBmatcher(0.8, True)
    for ps in _groups(PC.problems("frustum"), ("pyr",)):
        _run_frustum(m, ps)


def test_predict_scale_table_cache_evicts_and_refills():
    """Six pyramids in sequence on ONE matcher handle, then the first again: the per-handle cache of ratio-threshold tables holds four, so the first is
    evicted and built again.  Every level boundary of every pyramid (largest float of level n and the next float up) must come out as the oracle's."""
    from morb_slam_amd import ORBmatcher
    m = ORBmatcher(0.8, True)
    order = list(PC.PYRAMIDS) + list(PC.CACHE_PYRAMIDS)
    assert len(order) == 6
    for pyr in order + [order[0]]:
        p = PC.frustum_predict_scale(pyr) if pyr in PC.CACHE_PYRAMIDS else [q for q in PC.problems("frustum") if q["name"] == "predict_scale_" + pyr][0]
        _run_frustum(m, [p])


# ---- SearchByProjection(F, MapPoints) ------------------------------------------------------------------------------------------------------
def _run_mps(ps, cap):
    from morb_slam_amd import ORBmatcher
    ps = _with_edges(ps)
    mpCap = cap
    p0 = ps[0]
    kps, desc, cnt = _pool([(p["k"], p["d"]) for p in ps], cap)
    init = [_pad(p["init"], cap, SENT) for p in ps]
    rows = lambda key, fill=0: _stack([np.concatenate([p["q"][key], p["ghost"][key]]) for p in ps], mpCap, fill)
    trk = {k: rows(k) for k in ("inView", "depth", "projX", "projY", "projXR", "level", "viewCos")}
    nMP = np.array([len(p["q"]["projX"]) for p in ps], np.int32)
    m = ORBmatcher(p0["nnratio"], True)
    mt, nm = m.SearchByProjectionMapPoints(PC.params(p0["pyr"]), _cu(np.arange(len(ps), dtype=np.int32)), kps, desc, cnt, _stack([p["ur"] for p in ps], cap, -1),
                                           _stack([p["flag"] for p in ps], cap), _cu(nMP), trk, rows("isBad"), rows("mpDesc"), rows("hasObs"), p0["th"],
                                           p0["bFar"], p0["thFar"], matchF=_cu(np.stack(init)))
    mt, nm = mt.cpu().numpy(), nm.cpu().numpy()
    out = []
    for f, p in enumerate(ps):
        o = PC.oracle(p)
        assert int(nm[f]) == o["n"], (p["name"], int(nm[f]), o["n"])
        _table(mt[f], len(p["k"]), p, o, init[f])
        out += [mt[f, :len(p["k"])], int(nm[f])]
    return out


def test_search_by_projection_map_points(monkeypatch):
    _all_tiers("mps", _run_mps, _groups(PC.problems("mps"), ("pyr", "th", "nnratio", "bFar", "thFar")), monkeypatch, q_is_mp=True)


# ---- SearchByProjection(Cur, Last) and SearchByProjection(Cur, KF) ------------------------------------------------------------------------------
def _run_last(ps, cap, kf=False):
    from morb_slam_amd import ORBmatcher
    ps = _with_edges(ps)
    p0 = ps[0]
    nP = len(ps)
    frames = [(p["k"], p["d"]) for p in ps] + [(p["lastK"], np.zeros((len(p["lastK"]), 32), np.uint8)) for p in ps]
    kps, desc, cnt = _pool(frames, cap)
    cur = _cu(np.arange(nP, dtype=np.int32)); last = _cu(np.arange(nP, 2 * nP, dtype=np.int32))
    init = [_pad(p["init"], cap, SENT) for p in ps]
    m = ORBmatcher(0.9, p0["ori"])
    P = PC.params(p0["pyr"])
    common = (_stack([p["lastValid"] for p in ps], cap), _stack([p["lastXw"] for p in ps], cap))
    if kf:
        mc, nm = m.SearchByProjectionKeyFrame(P, cur, last, kps, desc, cnt, _stack([p["flag"] for p in ps], cap), _cu(np.stack([p["Tcw"] for p in ps])),
                                              _cu(np.stack([p["Ow"] for p in ps])), *common, _stack([p["maxD"] for p in ps], cap, 1),
                                              _stack([p["minD"] for p in ps], cap, 1), _stack([p["lastDesc"] for p in ps], cap), p0["th"], p0["orb"],
                                              matchCur=_cu(np.stack(init)))
    else:
        mc, nm = m.SearchByProjectionLastFrame(P, cur, last, kps, desc, cnt, _stack([p["ur"] for p in ps], cap, -1), _stack([p["flag"] for p in ps], cap),
                                               _cu(np.stack([p["Tcw"] for p in ps])), *common, _stack([p["lastDesc"] for p in ps], cap),
                                               _stack([p["lastObs"] for p in ps], cap), p0["th"], _cu(np.array([p["fwd"] for p in ps], np.uint8)),
                                               _cu(np.array([p["bwd"] for p in ps], np.uint8)), matchCur=_cu(np.stack(init)))
    mc, nm = mc.cpu().numpy(), nm.cpu().numpy()
    out = []
    for f, p in enumerate(ps):
        o = PC.oracle(p)
        assert int(nm[f]) == o["n"], (p["name"], int(nm[f]), o["n"])
        _table(mc[f], len(p["k"]), p, o, init[f])
        out += [mc[f, :len(p["k"])], int(nm[f])]
    return out


def test_search_by_projection_last_frame(monkeypatch):
    _all_tiers("last", _run_last, _groups(PC.problems("last"), ("pyr", "th", "ori")), monkeypatch)


def test_search_by_projection_keyframe(monkeypatch):
    _all_tiers("kf", lambda ps, cap: _run_last(ps, cap, kf=True), _groups(PC.problems("kf"), ("pyr", "th", "orb", "ori")), monkeypatch)


# ---- Fuse, both forms ---------------------------------------------------------------------------------------------------------------------------
def _run_fuse(ps, cap):
    from morb_slam_amd import ORBmatcher
    ps = _with_edges(ps)
    p0 = ps[0]
    mpCap = cap
    kps, desc, cnt = _pool([(p["k"], p["d"]) for p in ps], cap)
    nMP = np.array([len(p["Pw"]) for p in ps], np.int32)
    bi, bd = ORBmatcher(0.8, True).Fuse(PC.params(p0["pyr"]), _cu(np.arange(len(ps), dtype=np.int32)), kps, desc, cnt, _stack([p["ur"] for p in ps], cap, -1),
                                         _cu(np.stack([p["Tcw"] for p in ps])), _cu(np.stack([p["Ow"] for p in ps])), _cu(nMP),
                                         _stack([p["valid"] for p in ps], mpCap), _stack([p["Pw"] for p in ps], mpCap), _stack([p["normal"] for p in ps], mpCap),
                                         _stack([p["maxD"] for p in ps], mpCap, 1), _stack([p["minD"] for p in ps], mpCap, 1),
                                         _stack([p["mpDesc"] for p in ps], mpCap), th=p0["th"], sim3Form=p0["sim3Form"])
    bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    out = []
    for f, p in enumerate(ps):
        o = PC.oracle(p)
        n = int(nMP[f])
        _table(bi[f, :n], n, p, o)
        np.testing.assert_array_equal(bd[f, :n], o["dist"], err_msg=p["name"])
        out += [bi[f, :n], bd[f, :n]]
    return out


def test_fuse(monkeypatch):
    _all_tiers("fuse", _run_fuse, _groups(PC.problems("fuse"), ("pyr", "th", "sim3Form")), monkeypatch, q_is_mp=True)


# ---- SearchBySim3 ---------------------------------------------------------------------------------------------------------------------------
def _run_sim3dir(ps, cap):
    from morb_slam_amd import ORBmatcher
    p = ps[0]
    A, B, a, b = p["A"], p["B"], p["ptsA"], p["ptsB"]
    cutf = lambda fr, n: {k: v[:n] for k, v in fr.items()}
    # (keyframe 1, its points, keyframe 2, its points): the case, keyframe 2 empty, keyframe 1 with one feature
    probs = [(A, a, B, b), (A, a, cutf(B, 0), cutf(b, 0)), (cutf(A, 1), cutf(a, 1), B, b)]
    frames, i1, i2 = [], [], []
    for fa, _, fb, _ in probs:
        i1.append(len(frames)); frames.append((fa["k"], fa["d"])); i2.append(len(frames)); frames.append((fb["k"], fb["d"]))
    kps, desc, cnt = _pool(frames, cap)
    nP = len(probs)
    T7 = _cu(np.stack([PC.IDENTITY7] * nP))
    S7 = _cu(np.stack([p["S"]] * nP))
    tab = lambda j, key, fill=0: _stack([pr[j][key] for pr in probs], cap, fill)
    o = ORBmatcher(0.8, True).SearchBySim3(PC.params(p["pyr"]), _cu(np.array(i1, np.int32)), _cu(np.array(i2, np.int32)), kps, desc, cnt, T7, T7, S7, S7,
                                           tab(1, "valid"), tab(1, "Pw"), tab(1, "maxD", 1), tab(1, "minD", 1), tab(1, "mpDesc"),
                                           tab(3, "valid"), tab(3, "Pw"), tab(3, "maxD", 1), tab(3, "minD", 1), tab(3, "mpDesc"), p["th"])
    g1, g2, g12, nf = [x.cpu().numpy() for x in o]
    out = []
    for f, (fa, pa, fb, pb) in enumerate(probs):
        e = PC.oracle(dict(p, A=fa, B=fb, ptsA=pa, ptsB=pb))
        na, nb = len(fa["k"]), len(fb["k"])
        np.testing.assert_array_equal(g1[f, :na], e["v1"], err_msg="problem %d" % f); np.testing.assert_array_equal(g2[f, :nb], e["v2"], err_msg="problem %d" % f)
        np.testing.assert_array_equal(g12[f, :na], e["table"], err_msg="problem %d" % f)
        assert int(nf[f]) == e["n"]
        out += [g1[f, :na], g2[f, :nb], g12[f, :na]]
    np.testing.assert_array_equal(out[0], p["expect1"]); np.testing.assert_array_equal(out[1], p["expect2"]); np.testing.assert_array_equal(out[2], p["expect12"])
    return out


def test_search_by_sim3(monkeypatch):
    _all_tiers("sim3dir", _run_sim3dir, [PC.problems("sim3dir")], monkeypatch)


# ---- the searches without a k_search form: SearchByProjection(KF, Scw), SearchForInitialization, SearchForTriangulation -----------------------------
@pytest.mark.parametrize("cap", [128, 2032])
def test_search_by_projection_sim3(cap, monkeypatch):
    from morb_slam_amd import ORBmatcher
    assert T.entry_tier("sim3", cap, cap) == 3
    monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)
    for ps in _groups(PC.problems("sim3"), ("pyr", "th", "ratio", "manual")):
        ps = _with_edges(ps)
        p0 = ps[0]
        kps, desc, cnt = _pool([(p["k"], p["d"]) for p in ps], cap)
        nMP = np.array([len(p["Pw"]) for p in ps], np.int32)
        mf, nm = ORBmatcher(0.8, True).SearchByProjectionSim3(
            PC.params(p0["pyr"]), _cu(np.arange(len(ps), dtype=np.int32)), kps, desc, cnt, _cu(np.stack([p["Tcw"] for p in ps])),
            _cu(np.stack([p["Ow"] for p in ps])), _cu(nMP), _stack([p["valid"] for p in ps], cap), _stack([p["Pw"] for p in ps], cap),
            _stack([p["normal"] for p in ps], cap), _stack([p["maxD"] for p in ps], cap, 1), _stack([p["minD"] for p in ps], cap, 1),
            _stack([p["mpDesc"] for p in ps], cap), _stack([p["flag"] for p in ps], cap), int(p0["th"]), p0["ratio"], p0["manual"])
        mf, nm = mf.cpu().numpy(), nm.cpu().numpy()
        for f, p in enumerate(ps):
            o = PC.oracle(p)
            assert int(nm[f]) == o["n"], p["name"]
            _table(mf[f], len(p["k"]), p, o)


@pytest.mark.parametrize("cap", [128, 2032])
def test_search_for_initialization(cap, monkeypatch):
    from morb_slam_amd import ORBmatcher
    assert T.entry_tier("init", cap) == 3
    monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)
    for ps in _groups(PC.problems("init"), ("pyr", "nnratio", "win", "ori")):
        p0 = ps[0]
        one = {k: p0[k][:1] for k in ("k1", "d1", "prev")}
        ps = list(ps) + [dict(p0, k2=p0["k2"][:0], d2=p0["d2"][:0], expect=None, name=p0["name"] + "_empty_F2"),
                         dict(p0, expect=None, name=p0["name"] + "_one_query", **one)]
        frames, i1, i2 = [], [], []
        for p in ps:
            i1.append(len(frames)); frames.append((p["k1"], p["d1"])); i2.append(len(frames)); frames.append((p["k2"], p["d2"]))
        kps, desc, cnt = _pool(frames, cap)
        prev0 = np.full((len(ps), cap, 2), 3.5, np.float32)
        for f, p in enumerate(ps):
            prev0[f, :len(p["k1"])] = p["prev"]
        prev = _cu(prev0.copy())
        m12, nm = ORBmatcher(p0["nnratio"], p0["ori"]).SearchForInitialization(PC.params(p0["pyr"]), _cu(np.array(i1, np.int32)), _cu(np.array(i2, np.int32)),
                                                                                 kps, desc, cnt, prev, p0["win"])
        m12, nm, prevg = m12.cpu().numpy(), nm.cpu().numpy(), prev.cpu().numpy()
        for f, p in enumerate(ps):
            o = PC.oracle(p)
            n1 = len(p["k1"])
            assert int(nm[f]) == o["n"], p["name"]
            _table(m12[f], n1, p, o)
            assert prevg[f, :n1].tobytes() == o["prev"].tobytes() and prevg[f, n1:].tobytes() == prev0[f, n1:].tobytes(), p["name"]


def test_search_for_triangulation():
    from morb_slam_amd import ORBmatcher
    cap = 128
    for ps in _groups(PC.problems("tri"), ("pyr", "onlyStereo", "coarse", "ori")):
        p0 = ps[0]
        cutf = lambda fr, n: {k: v[:n] for k, v in fr.items()}
        ps = list(ps) + [dict(p0, F2=cutf(p0["F2"], 0), expect=None, name=p0["name"] + "_empty_F2"),
                         dict(p0, F1=cutf(p0["F1"], 1), expect=None, name=p0["name"] + "_one_query")]
        frames, i1, i2 = [], [], []
        for p in ps:
            i1.append(len(frames)); frames.append(p["F1"]); i2.append(len(frames)); frames.append(p["F2"])
        kps, desc, cnt = _pool([(fr["k"], fr["d"]) for fr in frames], cap)
        m12, nm = ORBmatcher(0.6, p0["ori"]).SearchForTriangulation(
            PC.params(p0["pyr"]), _cu(np.array(i1, np.int32)), _cu(np.array(i2, np.int32)), kps, desc, _stack([fr["node"] for fr in frames], cap, -1), cnt,
            _stack([fr["has"] for fr in frames], cap), _stack([fr["ur"] for fr in frames], cap, -1), np.stack([p["R12"] for p in ps]),
            np.stack([p["t12"] for p in ps]), np.stack([p["ep"] for p in ps]), p0["onlyStereo"], p0["coarse"])
        m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
        for f, p in enumerate(ps):
            o = PC.oracle(p)
            assert int(nm[f]) == o["n"], p["name"]
            _table(m12[f], len(p["F1"]["k"]), p, o)
