"""Projection searches on all three implementations of projection.hip (tests/search_tiers.py: 1 = k_search with LDS descriptors, 2 = k_search
with global descriptors, 3 = k_candidates + k_resolve / k_best_per_query), against the CPU oracle, tables and counts bit for bit.  Every case
asserts through the mirror the tier it means to run before it runs.

  entry \\ tier                     | 1                | 2                          | 3
  SearchByProjection(Cur, Last)     | same_data[last]  | same_data, kitti, dense    | same_data (4032, serial), c4, dense
  SearchByProjection(Cur, KF)       | same_data[kf]    | same_data, kitti, dense    | same_data (4032, serial), c4, dense
  SearchByProjection(F, MapPoints)  | same_data[mps]   | same_data, kitti, mp4000,  | same_data (4032, serial), c4, mp6000,
                                    |                  | dense                      | dense
  Fuse (both forms)                 | same_data[fuse*] | same_data, kitti, mp4000,  | same_data (4032, serial), c4, mp6000,
                                    |                  | dense                      | dense
  SearchBySim3 (each direction)     | same_data[sim3d] | same_data, kitti, dense    | same_data (4032, serial), c4, dense
  SearchByProjection(KF, Scw)       | (no k_search)    | (no k_search)              | same_data, kitti, c4, dense
  SearchForInitialization           | (no k_search)    | (no k_search)              | same_data, kitti, c4, init5000, dense
  (fisheye forms: test_fisheye_gpu.py)

same_data: the 1200-feature frames (cap 1232) as they are, padded into cap 2032 and cap 4032 tensors, and with MORB_SERIAL_RESOLVE set: the
tables must be identical to the cap-1232 run's and equal the oracle's.  Its batch mixes a full frame, a frame with count 0, a frame
without queries and a one-feature frame, and the in/out tables (LastFrame, KeyFrame, MapPoints) start with earlier assignments (some
features blocked, some not) and a sentinel past each frame's count.  kitti: 1241 x 376 at 2000 features; c4: 1920 x 1080 at 4000 features;
init5000: 752 x 480 at 5000 features; mp4000 / mp6000: 1200-feature frames with 4000 / 6000 map points; dense: windows that hold more than
SEARCH_CAP = 32 (tier 2: the query walks the grid again) and more than CAND_CAP = 128 candidates (tier 3: the keys are derived again)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import search_tiers as T
from matcher_scenes import make_batch, scene

pytestmark = pytest.mark.gpu

SENT = -7777           # rows past a frame's count in an in/out table: never written
ENTRIES = ["last", "kf", "mps", "fuse", "fuse_sim3", "sim3dir", "sim3", "init"]
_BATCHES = {}


class Scene:
    """A batch's frames as host arrays + stereo depth, plus two edge images: E0 (count 0) and E1 (one feature); device tensors per cap."""

    def __init__(self, batch):
        P, uR, dep = scene(batch)
        self.P, self.np_ = P, batch["npairs"]
        self.k = [o[1] for o in batch["ora"]]; self.d = [o[2] for o in batch["ora"]]
        nimg = len(self.k)
        self.ur = [uR[i // 2, :len(self.k[i])].cpu().numpy() if i % 2 == 0 else np.full(len(self.k[i]), -1, np.float32) for i in range(nimg)]
        self.z = [dep[i // 2, :len(self.k[i])].cpu().numpy() if i % 2 == 0 else np.zeros(len(self.k[i]), np.float32) for i in range(nimg)]
        src = 2 * self.np_                         # E1: the first feature of frame 0's shifted copy
        self.E0, self.E1 = nimg, nimg + 1
        self.k += [self.k[0][:0], self.k[src][:1]]; self.d += [self.d[0][:0], self.d[src][:1]]
        self.ur += [self.ur[0][:0], self.ur[src][:1]]; self.z += [self.z[0][:0], self.z[src][:1]]
        self.cap0 = batch["kps"].shape[1]
        self.W, self.H = batch["size"]
        self._dev = {}

    def n(self, i):
        return len(self.k[i])

    def dev(self, cap):
        import torch
        if cap not in self._dev:
            nimg = len(self.k)
            kps = np.zeros((nimg, cap, 28), np.uint8); desc = np.zeros((nimg, cap, 32), np.uint8)
            for i in range(nimg):
                kps[i, :self.n(i)] = self.k[i].view(np.uint8).reshape(-1, 28); desc[i, :self.n(i)] = self.d[i]
            cnt = np.array([self.n(i) for i in range(nimg)], np.int32)
            self._dev[cap] = tuple(torch.from_numpy(a).cuda() for a in (kps, desc, cnt))
        return self._dev[cap]

    def backproject(self, i):
        k, z = self.k[i], self.z[i]
        zz = np.where(z > 0, z, 1.0)
        X = np.stack([(k["x"] - self.P.cx) * zz / self.P.fx, (k["y"] - self.P.cy) * zz / self.P.fy, zz], 1).astype(np.float32)
        return X.reshape(-1, 3), z > 0

    def problems(self, edges=True):
        """(source image, target image, kind): kind 'noq' = a source without queries."""
        s = 2 * self.np_
        base = [(0, s, "full"), (s, 0, "full"), (2, s + 2, "full")]
        return base + [(0, self.E0, "full"), (0, s, "noq"), (0, self.E1, "full"), (self.E1, s, "full")] if edges else base


def _batch(w=752, h=480, nf=1200, npairs=2):
    key = (w, h, nf, npairs)
    if key not in _BATCHES:
        _BATCHES[key] = Scene(make_batch(w, h, nf, npairs))
    return _BATCHES[key]


def _pad(a, n, fill=0):
    a = np.asarray(a)
    return np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(a) if isinstance(a, list) else a)).cuda()


def _i32(a):
    import torch
    return torch.tensor(a, dtype=torch.int32, device="cuda")


def _prior(rng, n, cap, blocked):
    """An in/out table on entry: every blocked feature and ~30 % of the others hold an earlier assignment, SENT past the count."""
    t = np.full(cap, SENT, np.int32); t[:n] = -1
    has = (blocked[:n] != 0) | (rng.random(n) < 0.3)
    t[:n][has] = rng.integers(0, 5000, int(has.sum()))
    return t


def _pose(q, t):
    q = np.asarray(q, np.float64); q = q / np.linalg.norm(q)
    qc = q * np.array([-1, -1, -1, 1]); u = qc[:3]; uv = 2 * np.cross(u, -np.asarray(t)); Ow = -np.asarray(t) + qc[3] * uv + np.cross(u, uv)
    return np.concatenate([q, t]).astype(np.float32), Ow.astype(np.float32)


def _map_points(S, n, seed):
    """n map points in the world = camera of image 0: back-projected features of every left image, repeated with jitter beyond that."""
    rng = np.random.default_rng(seed)
    Xs, Ds, Ls = [], [], []
    for i in range(0, 4 * S.np_, 2):
        X, v = S.backproject(i)
        Xs.append(X[v]); Ds.append(S.d[i][v]); Ls.append(S.k[i]["octave"][v])
    X, D, L = np.concatenate(Xs), np.concatenate(Ds), np.concatenate(Ls)
    reps = -(-n // max(len(X), 1))
    X = np.concatenate([X] + [X * rng.uniform(0.98, 1.02, X.shape).astype(np.float32) for _ in range(reps - 1)])[:n]
    D = np.concatenate([D] * reps)[:n].copy(); L = np.concatenate([L] * reps)[:n]
    flip = rng.random(D.shape) < 0.01
    D[flip] ^= np.uint8(1 << 3)
    dist = np.linalg.norm(X, axis=1)
    maxD = (dist * 1.2 ** L * rng.uniform(0.9, 1.3, n)).astype(np.float32)
    normal = (X / np.maximum(dist[:, None], 1e-6) + rng.normal(0, 0.2, X.shape)).astype(np.float32)
    return dict(Xw=X.astype(np.float32), d=D, maxD=maxD, minD=(maxD / 1.2 ** 7).astype(np.float32), normal=normal,
                hasObs=(rng.random(n) < 0.9).astype(np.uint8), isBad=(rng.random(n) < 0.05).astype(np.uint8))


# ---- one runner per entry: GPU and oracle on the same problems; returns what the tiers must agree on ----------------------------------
def run_last(S, cap, mpCap, probs, th=7.0, fwd=0, bwd=0, ori=True, prior=True, seed=4):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    rng = np.random.default_rng(seed)
    A = {k: [] for k in ("valid", "Xw", "desc", "obs", "ur", "blk", "Tcw", "init")}
    for li, ci, kind in probs:
        X, v = S.backproject(li)
        v = v & (rng.random(S.n(li)) < 0.9) & (kind != "noq")
        A["valid"].append(_pad(v.astype(np.uint8), cap)); A["Xw"].append(_pad(X, cap)); A["desc"].append(_pad(S.d[li], cap))
        A["obs"].append(_pad((rng.random(S.n(li)) < 0.85).astype(np.uint8), cap))
        blk = _pad((rng.random(S.n(ci)) < 0.1).astype(np.uint8), cap)
        A["ur"].append(_pad(S.ur[ci], cap, -1)); A["blk"].append(blk)
        A["Tcw"].append(_pose([0.0, 0.002, 0.0, 1.0], [0.01, 0.0, 0.02])[0])
        A["init"].append(_prior(rng, S.n(ci), cap, blk) if prior else np.full(cap, -1, np.int32))
    m = ORBmatcher(0.9, ori)
    nP = len(probs)
    mc, nm = m.SearchByProjectionLastFrame(S.P, _i32([c for _, c, _ in probs]), _i32([s for s, _, _ in probs]), kps, desc, cnt, _cu(A["ur"]),
                                           _cu(A["blk"]), _cu(A["Tcw"]), _cu(A["valid"]), _cu(A["Xw"]), _cu(A["desc"]), _cu(A["obs"]), th,
                                           _cu(np.full(nP, fwd, np.uint8)), _cu(np.full(nP, bwd, np.uint8)), matchCur=_cu(A["init"]))
    mc, nm = mc.cpu().numpy(), nm.cpu().numpy()
    out, cleared = [], 0
    for p, (li, ci, _) in enumerate(probs):
        nl, nc = S.n(li), S.n(ci)
        Fo = O.make_frame(S.P, S.k[ci], S.d[ci], A["ur"][p][:nc])
        r, me = O.search_by_projection_last(Fo, A["blk"][p][:nc], A["Tcw"][p], S.k[li], A["valid"][p][:nl], A["Xw"][p][:nl], A["desc"][p][:nl],
                                            A["obs"][p][:nl], th, fwd, bwd, ori, match_init=A["init"][p][:nc])
        assert int(nm[p]) == r, (p, int(nm[p]), r)
        np.testing.assert_array_equal(mc[p, :nc], me, err_msg=f"problem {p}")
        np.testing.assert_array_equal(mc[p, nc:], A["init"][p][nc:], err_msg=f"problem {p}: rows past the count")
        cleared += int(((me == -1) & (A["init"][p][:nc] != -1)).sum())
        out += [mc[p, :nc], r]
    return out, cleared


def run_kf(S, cap, mpCap, probs, th=10.0, orb=100, ori=True, prior=True, seed=9):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    rng = np.random.default_rng(seed)
    A = {k: [] for k in ("valid", "Xw", "desc", "mx", "mn", "has", "Tcw", "Ow", "init")}
    for ki, ci, kind in probs:
        X, v = S.backproject(ki)
        v = v & (rng.random(S.n(ki)) < 0.9) & (kind != "noq")
        maxD = (np.linalg.norm(X, axis=1) * 1.2 ** S.k[ki]["octave"] * rng.uniform(0.9, 1.2, S.n(ki))).astype(np.float32)
        A["valid"].append(_pad(v.astype(np.uint8), cap)); A["Xw"].append(_pad(X, cap)); A["desc"].append(_pad(S.d[ki], cap))
        A["mx"].append(_pad(maxD, cap, 1)); A["mn"].append(_pad((maxD / 1.2 ** 7).astype(np.float32), cap, 1))
        has = _pad((rng.random(S.n(ci)) < 0.2).astype(np.uint8), cap)
        A["has"].append(has)
        Tcw, Ow = _pose([0.001, -0.002, 0.0, 1.0], [0.01, 0.0, -0.02])
        A["Tcw"].append(Tcw); A["Ow"].append(Ow)
        A["init"].append(_prior(rng, S.n(ci), cap, has) if prior else np.full(cap, -1, np.int32))
    m = ORBmatcher(0.9, ori)
    mc, nm = m.SearchByProjectionKeyFrame(S.P, _i32([c for _, c, _ in probs]), _i32([s for s, _, _ in probs]), kps, desc, cnt, _cu(A["has"]),
                                          _cu(A["Tcw"]), _cu(A["Ow"]), _cu(A["valid"]), _cu(A["Xw"]), _cu(A["mx"]), _cu(A["mn"]), _cu(A["desc"]),
                                          th, orb, matchCur=_cu(A["init"]))
    mc, nm = mc.cpu().numpy(), nm.cpu().numpy()
    out, cleared = [], 0
    for p, (ki, ci, _) in enumerate(probs):
        nk, nc = S.n(ki), S.n(ci)
        Fo = O.make_frame(S.P, S.k[ci], S.d[ci], None)
        r, me = O.search_by_projection_kf(Fo, A["has"][p][:nc], A["Tcw"][p], A["Ow"][p], S.k[ki], A["valid"][p][:nk], A["Xw"][p][:nk],
                                          A["mx"][p][:nk], A["mn"][p][:nk], A["desc"][p][:nk], th, orb, ori, match_init=A["init"][p][:nc])
        assert int(nm[p]) == r, (p, int(nm[p]), r)
        np.testing.assert_array_equal(mc[p, :nc], me, err_msg=f"problem {p}")
        np.testing.assert_array_equal(mc[p, nc:], A["init"][p][nc:], err_msg=f"problem {p}: rows past the count")
        cleared += int(((me == -1) & (A["init"][p][:nc] != -1)).sum())
        out += [mc[p, :nc], r]
    return out, cleared


def run_mps(S, cap, mpCap, probs, th=3.0, bFar=False, thFar=0.0, prior=True, nmp=None, seed=3):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    rng = np.random.default_rng(seed)
    nmp = mpCap if nmp is None else nmp
    M = _map_points(S, nmp, seed)
    nP = len(probs)
    ns = [0 if kind == "noq" else nmp for _, _, kind in probs]
    Rs, ts, Ows = [], [], []
    for p in range(nP):
        a = 0.01 * (p % 3)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        t = np.array([0.02, -0.01, 0.05], np.float32) * (p % 2)
        Rs.append(R.reshape(9)); ts.append(t); Ows.append((-(R.T @ t)).astype(np.float32))
    rep = lambda a, fill=0: _cu([_pad(a, mpCap, fill)] * nP)
    m = ORBmatcher(0.8, True)
    trk = m.isInFrustum(S.P, _cu(Rs), _cu(ts), _cu(Ows), _i32(ns), rep(M["Xw"]), rep(M["normal"]), rep(M["maxD"], 1), rep(M["minD"], 1), 0.5)
    blk = [_pad((rng.random(S.n(ci)) < 0.1).astype(np.uint8), cap) for _, ci, _ in probs]
    init = [_prior(rng, S.n(ci), cap, b) if prior else np.full(cap, -1, np.int32) for (_, ci, _), b in zip(probs, blk)]
    ur = [_pad(S.ur[ci], cap, -1) for _, ci, _ in probs]
    mt, nm = m.SearchByProjectionMapPoints(S.P, _i32([c for _, c, _ in probs]), kps, desc, cnt, _cu(ur), _cu(blk), _i32(ns), trk, rep(M["isBad"]),
                                           rep(M["d"]), rep(M["hasObs"]), th, bFar, thFar, matchF=_cu(init))
    mt, nm = mt.cpu().numpy(), nm.cpu().numpy()
    out = []
    for p, (_, ci, _) in enumerate(probs):
        n, nc = ns[p], S.n(ci)
        Fo = O.make_frame(S.P, S.k[ci], S.d[ci], ur[p][:nc])
        te = O.is_in_frustum(Fo, Rs[p].reshape(3, 3), ts[p], Ows[p], M["Xw"][:n], M["normal"][:n], M["maxD"][:n], M["minD"][:n], 0.5)
        for key in te:
            g = trk[key][p, :n].cpu().numpy()
            assert g.tobytes() == te[key].astype(g.dtype).tobytes(), key
        r, me = O.search_by_projection_mps(Fo, blk[p][:nc], te, M["isBad"][:n], M["d"][:n], M["hasObs"][:n], th, bFar, thFar, 0.8,
                                           match_init=init[p][:nc])
        assert int(nm[p]) == r, (p, int(nm[p]), r)
        np.testing.assert_array_equal(mt[p, :nc], me, err_msg=f"problem {p}")
        np.testing.assert_array_equal(mt[p, nc:], init[p][nc:], err_msg=f"problem {p}: rows past the count")
        out += [mt[p, :nc], r]
    return out, 0


def _kf_points(S, probs, mpCap, nmp, seed):
    """Map points (world = camera of image 0) searched in each problem's target keyframe, seen from a pose a few millimetres away."""
    from morb_slam_amd.synth import _quat_from_rotvec, _quat_rot
    M = _map_points(S, nmp, seed)
    rng = np.random.default_rng(seed + 1)
    ns = [0 if kind == "noq" else nmp for _, _, kind in probs]
    valid = [(rng.random(nmp) < 0.9).astype(np.uint8) for _ in probs]
    Ts, Ows = [], []
    for p in range(len(probs)):
        qp = _quat_from_rotvec(np.array([0.0004, -0.0006, 0.0003]) * (p % 2)); tp = np.array([0.002, -0.001, 0.003]) * (p % 2)
        Ts.append(np.concatenate([qp, tp]).astype(np.float32)); Ows.append((-_quat_rot(qp * np.array([-1, -1, -1, 1]), tp)).astype(np.float32))
    padm = lambda a, fill=0: _cu([_pad(a, mpCap, fill)] * len(probs))
    args = (_cu([_pad(v, mpCap) for v in valid]), padm(M["Xw"]), padm(M["normal"]), padm(M["maxD"], 1), padm(M["minD"], 1), padm(M["d"]))
    return M, ns, valid, Ts, Ows, args


def run_fuse(S, cap, mpCap, probs, th=3.0, sim3=False, nmp=None, seed=8):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    nmp = mpCap if nmp is None else nmp
    M, ns, valid, Ts, Ows, args = _kf_points(S, probs, mpCap, nmp, seed)
    invS = (1.0 / np.array(list(S.P.levelSigma2)[:S.P.nlevels], np.float32)).astype(np.float32)
    ur = [_pad(S.ur[ci], cap, -1.0) for _, ci, _ in probs]
    bi, bd = ORBmatcher(0.8, True).Fuse(S.P, _i32([c for _, c, _ in probs]), kps, desc, cnt, _cu(ur), _cu(Ts), _cu(Ows), _i32(ns), *args,
                                         th=th, sim3Form=sim3)
    bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    out = []
    for p, (_, ci, _) in enumerate(probs):
        n, nc = ns[p], S.n(ci)
        Fo = O.make_frame(S.P, S.k[ci], S.d[ci], S.ur[ci])
        ei, ed = O.fuse_search(Fo, invS, Ts[p], Ows[p], valid[p][:n], M["Xw"][:n], M["normal"][:n], M["maxD"][:n], M["minD"][:n], M["d"][:n], th, sim3)
        np.testing.assert_array_equal(bi[p, :n], ei, err_msg=f"problem {p}")
        np.testing.assert_array_equal(bd[p, :n], ed, err_msg=f"problem {p}")
        out += [bi[p, :n], bd[p, :n]]
    return out, 0


def run_fuse_sim3(S, cap, mpCap, probs, th=6.0, **kw):
    return run_fuse(S, cap, mpCap, probs, th=th, sim3=True, **kw)


def run_sim3(S, cap, mpCap, probs, th=8, ratio=0.8, manual=False, nmp=None, seed=12):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    nmp = mpCap if nmp is None else nmp
    M, ns, valid, Ts, Ows, args = _kf_points(S, probs, mpCap, nmp, seed)
    rng = np.random.default_rng(seed)
    matched = [_pad((rng.random(S.n(ci)) < 0.1).astype(np.uint8), cap) for _, ci, _ in probs]
    mf, nm = ORBmatcher(0.8, True).SearchByProjectionSim3(S.P, _i32([c for _, c, _ in probs]), kps, desc, cnt, _cu(Ts), _cu(Ows), _i32(ns), *args,
                                                          _cu(matched), th, ratio, manual)
    mf, nm = mf.cpu().numpy(), nm.cpu().numpy()
    out = []
    for p, (_, ci, _) in enumerate(probs):
        n, nc = ns[p], S.n(ci)
        Fo = O.make_frame(S.P, S.k[ci], S.d[ci], None)
        r, me = O.search_by_projection_sim3(Fo, Ts[p], Ows[p], valid[p][:n], M["Xw"][:n], M["normal"][:n], M["maxD"][:n], M["minD"][:n],
                                            M["d"][:n], matched[p][:nc], th, ratio, manual)
        assert int(nm[p]) == r, (p, int(nm[p]), r)
        np.testing.assert_array_equal(mf[p, :nc], me, err_msg=f"problem {p}")
        out += [mf[p, :nc], r]
    return out, 0


def run_sim3dir(S, cap, mpCap, probs, th=7.5, seed=13):
    """SearchBySim3 between keyframe 1 = the source image (pose identity) and keyframe 2 = the target (a nearby pose), each with the
    stereo back-projections of its own features."""
    from morb_slam_amd import ORBmatcher
    from morb_slam_amd.synth import _quat_from_R, _quat_from_rotvec, _quat_rot
    kps, desc, cnt = S.dev(cap)
    rng = np.random.default_rng(seed)
    q2 = _quat_from_rotvec(np.array([0.002, -0.004, 0.001])); t2 = np.array([-0.03, -0.015, 0.01])
    R2 = np.array([_quat_rot(q2, e) for e in np.eye(3)]).T
    def sim8(R, t, s):
        return np.concatenate([_quat_from_R(R) * np.sqrt(s), t]).astype(np.float32)
    s = 1.01
    R12 = R2.T; t12 = -(R12 @ t2)
    S12 = sim8(R12, t12, s); R21 = R12.T; S21 = sim8(R21, -(R21 @ t12) / s, 1.0 / s)
    T1 = np.array([0, 0, 0, 1, 0, 0, 0], np.float32); T2 = np.concatenate([q2, t2]).astype(np.float32)
    K = {k: [] for k in ("v1", "X1", "mx1", "mn1", "d1", "v2", "X2", "mx2", "mn2", "d2")}
    for a, b, kind in probs:
        for tag, img, T in (("1", a, None), ("2", b, (q2, t2))):
            X, v = S.backproject(img)
            if T is not None:        # camera-2 coordinates -> world
                qinv = T[0] * np.array([-1, -1, -1, 1])
                X = np.array([_quat_rot(qinv, x - T[1]) for x in X], np.float32).reshape(-1, 3)
            v = v & (rng.random(S.n(img)) < 0.85) & (kind != "noq" or tag == "2")
            dist = np.linalg.norm(S.backproject(img)[0], axis=1)
            maxD = (dist * 1.2 ** S.k[img]["octave"] * rng.uniform(0.9, 1.3, S.n(img))).astype(np.float32)
            K["v" + tag].append(_pad(v.astype(np.uint8), cap)); K["X" + tag].append(_pad(X, cap)); K["d" + tag].append(_pad(S.d[img], cap))
            K["mx" + tag].append(_pad(maxD, cap, 1)); K["mn" + tag].append(_pad((maxD / 1.2 ** 7).astype(np.float32), cap, 1))
    nP = len(probs)
    o = ORBmatcher(0.8, True).SearchBySim3(S.P, _i32([a for a, _, _ in probs]), _i32([b for _, b, _ in probs]), kps, desc, cnt,
                                           _cu([T1] * nP), _cu([T2] * nP), _cu([S12] * nP), _cu([S21] * nP),
                                           *[_cu(K[k]) for k in ("v1", "X1", "mx1", "mn1", "d1", "v2", "X2", "mx2", "mn2", "d2")], th)
    g1, g2, g12, nf = [x.cpu().numpy() for x in o]
    out = []
    for p, (a, b, _) in enumerate(probs):
        na, nb = S.n(a), S.n(b)
        FB = O.make_frame(S.P, S.k[b], S.d[b], None); FA = O.make_frame(S.P, S.k[a], S.d[a], None)
        e1 = O.search_by_sim3_dir(FB, T1, S21, K["v1"][p][:na], K["X1"][p][:na], K["mx1"][p][:na], K["mn1"][p][:na], K["d1"][p][:na], th)
        e2 = O.search_by_sim3_dir(FA, T2, S12, K["v2"][p][:nb], K["X2"][p][:nb], K["mx2"][p][:nb], K["mn2"][p][:nb], K["d2"][p][:nb], th)
        np.testing.assert_array_equal(g1[p, :na], e1, err_msg=f"problem {p}")
        np.testing.assert_array_equal(g2[p, :nb], e2, err_msg=f"problem {p}")
        e12 = np.array([i2 if (i2 >= 0 and e2[i2] == i1) else -1 for i1, i2 in enumerate(e1)], np.int32)
        np.testing.assert_array_equal(g12[p, :na], e12, err_msg=f"problem {p}")
        assert int(nf[p]) == int((e12 >= 0).sum())
        out += [g1[p, :na], g2[p, :nb], g12[p, :na]]
    return out, 0


def run_init(S, cap, mpCap, probs, win=100, ratio=0.9, ori=True, seed=0):
    from morb_slam_amd import ORBmatcher
    kps, desc, cnt = S.dev(cap)
    prev0 = np.zeros((len(probs), cap, 2), np.float32)
    pairs = []
    for p, (a, b, kind) in enumerate(probs):
        if kind == "noq":
            a = S.E0                 # F1 without features: no queries
        prev0[p, :S.n(a), 0] = S.k[a]["x"]; prev0[p, :S.n(a), 1] = S.k[a]["y"]
        pairs.append((a, b))
    prev = _cu(prev0.copy())
    m12, nm = ORBmatcher(ratio, ori).SearchForInitialization(S.P, _i32([a for a, _ in pairs]), _i32([b for _, b in pairs]), kps, desc, cnt, prev, win)
    m12, nm, prevg = m12.cpu().numpy(), nm.cpu().numpy(), prev.cpu().numpy()
    out = []
    for p, (a, b) in enumerate(pairs):
        na = S.n(a)
        r, me, pe = O.search_for_initialization(S.k[a], S.d[a], O.make_frame(S.P, S.k[b], S.d[b], None), prev0[p, :na], win, ratio, ori)
        assert int(nm[p]) == r, (p, int(nm[p]), r)
        np.testing.assert_array_equal(m12[p, :na], me, err_msg=f"problem {p}")
        assert prevg[p, :na].tobytes() == pe.tobytes()
        assert prevg[p, na:].tobytes() == prev0[p, na:].tobytes()
        out += [m12[p, :na], r]
    return out, 0


RUN = dict(last=run_last, kf=run_kf, mps=run_mps, fuse=run_fuse, fuse_sim3=run_fuse_sim3, sim3dir=run_sim3dir, sim3=run_sim3, init=run_init)
MIRROR = dict(fuse_sim3="fuse")          # the mirror's entry names


def _run(entry, S, cap, mpCap, want_tier, monkeypatch, serial=False, **kw):
    """Assert the tier through the mirror, run the entry (GPU vs oracle inside), return its tables."""
    import torch
    assert T.entry_tier(MIRROR.get(entry, entry), cap, mpCap, serial) == want_tier, (entry, cap, mpCap, serial)
    if serial:
        monkeypatch.setenv("MORB_SERIAL_RESOLVE", "1")
    else:
        monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)
    try:
        out = RUN[entry](S, cap, mpCap, S.problems(), **kw)
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("MORB_SERIAL_RESOLVE", raising=False)
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


# mpCap of the map-point searches in the same-data cases: the frame capacity (so the padded runs move to tiers 2 and 3 too)
_QSEARCH = ("mps", "fuse", "fuse_sim3", "sim3")


@pytest.mark.parametrize("entry", ENTRIES)
def test_same_data_every_tier(entry, monkeypatch):
    S = _batch()
    assert S.cap0 == 1232
    fast = entry not in ("sim3", "init")
    runs = [(1232, 1 if fast else 3, False), (2032, 2 if fast else 3, False), (4032, 3, False), (1232, 3, True)]
    first, cleared = None, 0
    for cap, tier, serial in runs:
        mpCap = cap if entry in _QSEARCH else None
        nmp = 1232 if entry in _QSEARCH else None
        kw = {"nmp": nmp} if nmp else {}
        out, c = _run(entry, S, cap, mpCap, tier, monkeypatch, serial, **kw)
        cleared += c
        if first is None:
            first = out
        else:
            _same(first, out)
    if entry in ("last", "kf"):
        assert cleared > 0     # the rotation filter cleared entries that held an earlier assignment, in every run alike


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["kitti", "c4"])
def test_real_shapes(entry, shape, monkeypatch):
    w, h, nf, npairs = (1241, 376, 2000, 2) if shape == "kitti" else (1920, 1080, 4000, 1)
    S = _batch(w, h, nf, npairs)
    cap = S.cap0
    assert cap == T.frame_cap(nf)
    mpCap = 2048 if shape == "kitti" else 4096
    fast = entry not in ("sim3", "init")
    want = (2 if shape == "kitti" else 3) if fast else 3
    kw = dict(th=10.0) if entry in ("mps",) else {}
    _run(entry, S, cap, mpCap if entry in _QSEARCH else None, want, monkeypatch, **kw)


def test_init_5000_features(monkeypatch):
    """EuRoC monocular initialisation: the init extractor asks for 5 * nFeatures = 5000 features (Tracking.cc)."""
    S = _batch(752, 480, 5000, 1)
    assert S.cap0 == 5032
    _run("init", S, S.cap0, None, 3, monkeypatch)
    _run("init", S, S.cap0, None, 3, monkeypatch, win=20, ratio=0.7, ori=False)


@pytest.mark.parametrize("entry,nmp,tier", [("mps", 4000, 2), ("mps", 6000, 3), ("fuse", 4000, 2), ("fuse", 6000, 3),
                                            ("fuse_sim3", 4000, 2), ("fuse_sim3", 6000, 3)])
def test_large_local_maps(entry, nmp, tier, monkeypatch):
    """SearchLocalPoints / Fuse on 1200-feature frames with a long sequence's local map."""
    S = _batch()
    _run(entry, S, S.cap0, nmp, tier, monkeypatch)


# wide windows: every query of a low level sees more than 128 candidates (tier 3 derives the keys again) and more than 32 (tier 2 walks the
# grid again); a window of half size >= the image width holds every feature of its levels
_DENSE = dict(last=dict(th=800.0, fwd=1), kf=dict(th=800.0), mps=dict(th=330.0), fuse_sim3=dict(th=800.0), sim3=dict(th=800),
              sim3dir=dict(th=800.0), init=dict(win=800), fuse=dict(th=45.0))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("cap", [2032, 4032])
def test_dense_windows(entry, cap, monkeypatch):
    S = _batch()
    k = S.k[2 * S.np_]
    assert int((k["octave"] <= 1).sum()) > 128 and S.W <= 800
    fast = entry not in ("sim3", "init")
    tier = 2 if (cap == 2032 and fast) else 3
    mpCap = cap if entry in _QSEARCH else None
    kw = dict(_DENSE[entry])
    if entry in _QSEARCH:
        kw["nmp"] = 1232
    a = _run(entry, S, cap, mpCap, tier, monkeypatch, **kw)
    if cap == 4032 and fast:            # and the same tables from the serial replay at the other capacity
        b = _run(entry, S, 2032, 2032 if entry in _QSEARCH else None, 3, monkeypatch, serial=True, **kw)
        _same(a[0], b[0])


def test_initialization_refuses_more_than_8192_features():
    """SearchForInitialization keeps two ints per feature of F2 in LDS (64 KB): a larger capacity is refused with MORB_ERR_UNSUPPORTED
    before anything is launched, so the outputs keep what they held."""
    import torch
    from morb_slam_amd import ORBmatcher
    from morb_slam_amd.capi import ptr
    S = _batch()
    cap = 8200
    assert cap * 8 > 64 * 1024
    kps, desc, cnt = S.dev(cap)
    m = ORBmatcher(0.9, True)
    m12 = torch.full((2, cap), SENT, dtype=torch.int32, device="cuda"); nm = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    prev = torch.full((2, cap, 2), 3.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    img1, img2 = _i32([0, 2]), _i32([4, 6])
    rc = m._L.morb_search_for_initialization_batch(m._h, C.byref(S.P), 2, ptr(img1), ptr(img2), cap, ptr(cnt), ptr(kps), ptr(desc),
                                                   ptr(prev), 100, C.c_float(0.9), 1, ptr(m12), ptr(nm), None)
    torch.cuda.synchronize()
    assert rc == -4   # MORB_ERR_UNSUPPORTED
    assert (m12.cpu().numpy() == SENT).all() and (nm.cpu().numpy() == SENT).all() and (prev.cpu().numpy() == 3.5).all()
